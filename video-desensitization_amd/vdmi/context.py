"""Python handle over one libvdmi context (one GPU, one stream).

Frames may be numpy uint8 [n,h,w,3] (host) or torch uint8 tensors on the
context's GPU (device); torch is used only to hand over device pointers and
streams (plumbing), never for compute.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _row_padded(t):
    """A torch [n,h,w,3] view whose rows are padded (t = big[:, :, :w]): packed pixels,
    row pitch stride(1) >= 3w, frame i at base + i*h*pitch -- the C-ABI's frame layout."""
    n, h, w, _ = t.shape
    st = t.stride()
    return st[3] == 1 and st[2] == 3 and st[1] >= 3 * w and (n == 1 or st[0] == h * st[1])


def _frames_arg(frames, pitched=False):
    """-> (pointer, n, h, w, pitch, where, keepalive). pitched: a torch view with padded
    rows is passed as it is (its row pitch) instead of being packed into a copy."""
    if _is_torch(frames):
        if frames.dtype.__str__() != "torch.uint8" or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be uint8 [n,h,w,3]")
        if pitched and not frames.is_contiguous() and _row_padded(frames):
            n, h, w, _ = frames.shape
            where = _lib.VD_DEVICE if frames.is_cuda else _lib.VD_HOST
            return frames.data_ptr(), n, h, w, frames.stride(1), where, frames
        if not frames.is_contiguous():
            frames = frames.contiguous()
        n, h, w, _ = frames.shape
        where = _lib.VD_DEVICE if frames.is_cuda else _lib.VD_HOST
        return frames.data_ptr(), n, h, w, w * 3, where, frames
    a = np.ascontiguousarray(frames, dtype=np.uint8)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError("frames must be uint8 [n,h,w,3]")
    n, h, w, _ = a.shape
    return a.ctypes.data, n, h, w, w * 3, _lib.VD_HOST, a


def _nv12_arg(frames, height=None, matrix="bt709", range="limited", writable=False):
    """NV12 frames -> (vd_nv12, n, h, w, where, keepalive). frames: uint8 [n, rows, w] (or [rows, w]),
    numpy or torch, host or device: `rows` luma rows followed by rows / 2 chroma rows of interleaved
    U, V. rows = 3h/2 is the packed layout; with height=h a taller rows = 3H/2 describes a luma
    plane padded to H >= h rows (a decoder's aligned height: the chroma plane starts at row H). A
    torch view with padded rows or frames (big[:, :, :w], big[:, :rows]) is passed by its strides.
    writable: the call writes the frames, so a layout that would need a packed copy is a ValueError."""
    if matrix not in _lib.NV12_MATRICES:
        raise ValueError(f"matrix {matrix!r}: expected 'bt601' or 'bt709'")
    if range not in _lib.NV12_RANGES:
        raise ValueError(f"range {range!r}: expected 'limited' or 'full'")
    if _is_torch(frames):
        t = frames if frames.dim() == 3 else frames[None]
        if t.dtype.__str__() != "torch.uint8" or t.dim() != 3:
            raise ValueError("NV12 frames must be uint8 [n, rows, w]")
        n, rows, w = t.shape
        st = t.stride()
        if not (st[2] == 1 and st[1] >= w and (n == 1 or st[0] >= rows * st[1])):
            if writable:
                raise ValueError("NV12 out: a torch tensor with unit column stride and row-major frames is needed")
            t = t.contiguous()
            st = t.stride()
        base, pitch, fstride = t.data_ptr(), st[1], (st[0] if n > 1 else rows * st[1])
        where = _lib.VD_DEVICE if t.is_cuda else _lib.VD_HOST
        keep = t
    else:
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        if writable and a is not frames:
            raise ValueError("NV12 out: a C-contiguous uint8 numpy array is needed")
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("NV12 frames must be uint8 [n, rows, w]")
        n, rows, w = a.shape
        base, pitch, fstride, where, keep = a.ctypes.data, w, rows * w, _lib.VD_HOST, a
    if rows % 3:
        raise ValueError(f"NV12 frames of {rows} rows: expected 3/2 of an even (padded) height")
    hpad = rows // 3 * 2
    h = hpad if height is None else int(height)
    if h > hpad:
        raise ValueError(f"height {h} exceeds the {hpad} luma rows that {rows} rows hold")
    d = _lib.vd_nv12(base, pitch, hpad * pitch, fstride, _lib.NV12_MATRICES[matrix], _lib.NV12_RANGES[range])
    return d, n, h, w, where, keep


def nv12_to_rgb(frames, matrix="bt709", range="limited", height=None):
    """vd_nv12_to_rgb (host only, no GPU: the routine the kernels' conversion is compiled from): host
    NV12 frames (the forms of Context.process_nv12) -> uint8 [n, h, w, 3]."""
    if _is_torch(frames):
        frames = frames.cpu()
    d, n, h, w, _, keep = _nv12_arg(frames, height, matrix, range)
    out = np.empty((n, max(h, 0), max(w, 0), 3), np.uint8)
    check(_lib.load().vd_nv12_to_rgb(ctypes.byref(d), n, h, w, ptr(out), w * 3))
    del keep
    return out


class Yuv420:
    """8-bit 4:2:0 frames anywhere in one buffer (the C-ABI's vd_yuv420): padded pools, planes in
    separate regions of one allocation, any of I420 / YV12 / NV12 / NV21. buffer: a uint8 numpy array
    or torch tensor (host or device), contiguous, of any shape; offsets in bytes from its first byte,
    which is frame 0's first luma byte. Luma rows are `pitch` bytes apart; U / V sample (cy, cx) of a
    frame is at u_offset / v_offset + cy * chroma_pitch + cx * chroma_step; frame i starts at
    i * frame_stride. n defaults to the number of whole frames the buffer holds."""

    def __init__(self, buffer, h, w, pitch, u_offset, v_offset, chroma_pitch, chroma_step, frame_stride, n=None):
        if _is_torch(buffer):
            if buffer.dtype.__str__() != "torch.uint8" or not buffer.is_contiguous():
                raise ValueError("Yuv420: a contiguous uint8 buffer is needed")
            nbytes, self._ptr = buffer.numel(), buffer.data_ptr()
            self.where = _lib.VD_DEVICE if buffer.is_cuda else _lib.VD_HOST
        else:
            if not (isinstance(buffer, np.ndarray) and buffer.dtype == np.uint8 and buffer.flags.c_contiguous):
                raise ValueError("Yuv420: a contiguous uint8 buffer is needed")
            nbytes, self._ptr, self.where = buffer.size, buffer.ctypes.data, _lib.VD_HOST
        self.buffer = buffer
        self.h, self.w, self.pitch = int(h), int(w), int(pitch)
        self.u_offset, self.v_offset = int(u_offset), int(v_offset)
        self.chroma_pitch, self.chroma_step, self.frame_stride = int(chroma_pitch), int(chroma_step), int(frame_stride)
        if min(self.h, self.w, self.pitch, self.chroma_pitch, self.frame_stride) <= 0 or min(self.u_offset, self.v_offset) < 0:
            raise ValueError("Yuv420: positive sizes and pitches, non-negative offsets needed")
        crow = self.w // 2 * max(self.chroma_step, 1)
        cend = max(self.u_offset, self.v_offset) + (max(self.h // 2, 1) - 1) * self.chroma_pitch + \
            (crow if self.chroma_step != 2 else crow - 1)
        end = max((self.h - 1) * self.pitch + self.w, cend)
        fit = 0 if nbytes < end else 1 + (nbytes - end) // self.frame_stride
        self.n = fit if n is None else int(n)
        if self.n < 1 or self.n > fit:
            raise ValueError(f"Yuv420: the buffer of {nbytes} bytes holds {fit} such frames (n = {self.n})")

    def struct(self, matrix="bt709", range="limited"):
        return _lib.vd_yuv420(self._ptr, self.pitch, self.u_offset, self.v_offset, self.chroma_pitch, self.frame_stride,
                              self.chroma_step, _lib.NV12_MATRICES[matrix], _lib.NV12_RANGES[range])


def _yuv420_arg(frames, layout="i420", height=None, matrix="bt709", range="limited", writable=False):
    """4:2:0 frames -> (vd_yuv420, n, h, w, where, keepalive). frames: a Yuv420, or uint8 [n, rows, w]
    (or [rows, w]) in `layout`: "nv12" / "nv21" as _nv12_arg takes NV12 frames (interleaved U, V /
    V, U pairs); "i420" / "yv12" packed planar, rows = 3h/2: h luma rows, then the first chroma
    plane's h/2 * w/2 bytes, then the second's (U then V / V then U) -- the array PyAV's
    to_ndarray(format="yuv420p") gives. With height=h a taller rows = 3H/2 is a luma plane padded to H
    rows (each chroma plane then holds H/2 rows)."""
    if matrix not in _lib.NV12_MATRICES:
        raise ValueError(f"matrix {matrix!r}: expected 'bt601' or 'bt709'")
    if range not in _lib.NV12_RANGES:
        raise ValueError(f"range {range!r}: expected 'limited' or 'full'")
    if isinstance(frames, Yuv420):
        return frames.struct(matrix, range), frames.n, frames.h, frames.w, frames.where, frames
    if layout not in _lib.YUV420_LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {_lib.YUV420_LAYOUTS}")
    planar = layout in ("i420", "yv12")
    if planar and _is_torch(frames) and frames.dim() in (2, 3) and frames.stride(-2) != frames.shape[-1]:
        if writable:
            raise ValueError("planar 4:2:0 out: rows of exactly w bytes are needed (or pass a Yuv420)")
        frames = frames.contiguous()
    d, n, h, w, where, keep = _nv12_arg(frames, height, matrix, range, writable)
    first, second = d.uv_offset, d.uv_offset + 1
    cpitch, step = d.pitch, 2
    if planar:
        if w % 2 or (d.uv_offset // d.pitch) % 2:
            raise ValueError("planar 4:2:0 frames: an even width and an even (padded) luma height are needed")
        cpitch, step = w // 2, 1
        second = first + (d.uv_offset // d.pitch // 2) * cpitch
    u, v = (first, second) if layout in ("i420", "nv12") else (second, first)
    y = _lib.vd_yuv420(d.base, d.pitch, u, v, cpitch, d.frame_stride, step, d.matrix, d.range)
    return y, n, h, w, where, keep


def yuv420_to_rgb(frames, layout="i420", matrix="bt709", range="limited", height=None):
    """vd_yuv420_to_rgb (host only, no GPU: the routine the kernels' conversion is compiled from): host
    4:2:0 frames in any layout (the forms of Context.process_yuv420) -> uint8 [n, h, w, 3]."""
    if _is_torch(frames):
        frames = frames.cpu()
    d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
    if where != _lib.VD_HOST:
        raise ValueError("yuv420_to_rgb() converts host frames")
    out = np.empty((n, max(h, 0), max(w, 0), 3), np.uint8)
    check(_lib.load().vd_yuv420_to_rgb(ctypes.byref(d), n, h, w, ptr(out), w * 3))
    del keep
    return out


class Yuv420_16:
    """10- or 12-bit 4:2:0 frames anywhere in one buffer (the C-ABI's vd_yuv420_16): P010 / P012,
    yuv420p10le / yuv420p12le and their V-first variants, padded or not. buffer: a contiguous numpy
    array or torch tensor (host or device) of uint16 (torch: uint16 or int16), or of uint8 -- as Yuv420
    takes buffers; all offsets and pitches are in BYTES from its first byte, which is frame 0's first
    luma word; chroma_step counts samples (1 planar, 2 interleaved pairs). A word's value is
    (word >> shift) & (2**depth - 1). n defaults to the number of whole frames the buffer holds."""

    _TORCH = {"torch.uint8": 1, "torch.uint16": 2, "torch.int16": 2}

    def __init__(self, buffer, h, w, pitch, u_offset, v_offset, chroma_pitch, chroma_step, frame_stride, depth=10,
                 shift=0, n=None):
        if _is_torch(buffer):
            item = self._TORCH.get(buffer.dtype.__str__())
            if item is None or not buffer.is_contiguous():
                raise ValueError("Yuv420_16: a contiguous uint16 or uint8 buffer is needed")
            nbytes, self._ptr = buffer.numel() * item, buffer.data_ptr()
            self.where = _lib.VD_DEVICE if buffer.is_cuda else _lib.VD_HOST
        else:
            if not (isinstance(buffer, np.ndarray) and buffer.dtype in (np.uint8, np.uint16) and buffer.flags.c_contiguous):
                raise ValueError("Yuv420_16: a contiguous uint16 or uint8 buffer is needed")
            nbytes, self._ptr, self.where = buffer.nbytes, buffer.ctypes.data, _lib.VD_HOST
        self.buffer = buffer
        self.h, self.w, self.pitch = int(h), int(w), int(pitch)
        self.u_offset, self.v_offset = int(u_offset), int(v_offset)
        self.chroma_pitch, self.chroma_step, self.frame_stride = int(chroma_pitch), int(chroma_step), int(frame_stride)
        self.depth, self.shift = int(depth), int(shift)
        if min(self.h, self.w, self.pitch, self.chroma_pitch, self.frame_stride) <= 0 or min(self.u_offset, self.v_offset) < 0:
            raise ValueError("Yuv420_16: positive sizes and pitches, non-negative offsets needed")
        crow = self.w * max(self.chroma_step, 1)        # bytes of a chroma row
        cend = max(self.u_offset, self.v_offset) + (max(self.h // 2, 1) - 1) * self.chroma_pitch + \
            (crow if self.chroma_step != 2 else crow - 2)
        end = max((self.h - 1) * self.pitch + 2 * self.w, cend)
        fit = 0 if nbytes < end else 1 + (nbytes - end) // self.frame_stride
        self.n = fit if n is None else int(n)
        if self.n < 1 or self.n > fit:
            raise ValueError(f"Yuv420_16: the buffer of {nbytes} bytes holds {fit} such frames (n = {self.n})")

    def struct(self, matrix="bt709", range="limited"):
        return _lib.vd_yuv420_16(self._ptr, self.pitch, self.u_offset, self.v_offset, self.chroma_pitch, self.frame_stride,
                                 self.chroma_step, _lib.NV12_MATRICES[matrix], _lib.NV12_RANGES[range], self.depth,
                                 self.shift)


def _yuv420_16_arg(frames, layout="i420", depth=10, shift=None, height=None, matrix="bt709", range="limited",
                   writable=False):
    """10- / 12-bit 4:2:0 frames -> (vd_yuv420_16, n, h, w, where, keepalive). frames: a Yuv420_16, or
    packed uint16 [n, rows, w] (or [rows, w]; torch: uint16 or int16) in `layout` as _yuv420_arg lays
    8-bit frames out, a word per sample. shift None: 0 for the planar layouts, 16 - depth for the
    interleaved ones (the P010 convention). height as in _yuv420_arg."""
    if matrix not in _lib.NV12_MATRICES:
        raise ValueError(f"matrix {matrix!r}: expected 'bt601' or 'bt709'")
    if range not in _lib.NV12_RANGES:
        raise ValueError(f"range {range!r}: expected 'limited' or 'full'")
    if isinstance(frames, Yuv420_16):
        return frames.struct(matrix, range), frames.n, frames.h, frames.w, frames.where, frames
    if layout not in _lib.YUV420_LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected one of {_lib.YUV420_LAYOUTS}")
    planar = layout in ("i420", "yv12")
    if _is_torch(frames):
        t = frames if frames.dim() == 3 else frames[None]
        if t.dtype.__str__() not in ("torch.uint16", "torch.int16") or t.dim() != 3:
            raise ValueError("16-bit 4:2:0 frames must be uint16 [n, rows, w]")
        if not t.is_contiguous():
            if writable:
                raise ValueError("16-bit 4:2:0 out: a contiguous tensor is needed (or pass a Yuv420_16)")
            t = t.contiguous()
        base, where, keep = t.data_ptr(), (_lib.VD_DEVICE if t.is_cuda else _lib.VD_HOST), t
        n, rows, w = t.shape
    else:
        a = np.ascontiguousarray(frames, dtype=np.uint16)
        if writable and a is not frames:
            raise ValueError("16-bit 4:2:0 out: a C-contiguous uint16 numpy array is needed")
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("16-bit 4:2:0 frames must be uint16 [n, rows, w]")
        n, rows, w = a.shape
        base, where, keep = a.ctypes.data, _lib.VD_HOST, a
    if rows % 3 or w % 2 or (planar and (rows // 3 * 2) % 2):
        raise ValueError(f"16-bit 4:2:0 frames of {rows} rows x {w}: expected 3/2 of an even (padded) height and an even width")
    hpad = rows // 3 * 2
    h = hpad if height is None else int(height)
    if h > hpad:
        raise ValueError(f"height {h} exceeds the {hpad} luma rows that {rows} rows hold")
    pitch = 2 * w
    first = hpad * pitch
    if planar:
        cpitch, step, second = w, 1, first + (hpad // 2) * w
    else:
        cpitch, step, second = pitch, 2, first + 2
    u, v = (first, second) if layout in ("i420", "nv12") else (second, first)
    if shift is None:
        shift = 0 if planar else 16 - int(depth)
    d = _lib.vd_yuv420_16(base, pitch, u, v, cpitch, rows * pitch, step, _lib.NV12_MATRICES[matrix],
                          _lib.NV12_RANGES[range], int(depth), int(shift))
    return d, n, h, w, where, keep


def yuv420_16_to_rgb(frames, layout="i420", depth=10, shift=None, matrix="bt709", range="limited", height=None):
    """vd_yuv420_16_to_rgb (host only, no GPU): host 10- / 12-bit 4:2:0 frames (the forms of
    Context.process_yuv420_16) -> uint8 [n, h, w, 3], the conversion of their 8-bit picture D(S)."""
    if _is_torch(frames):
        frames = frames.cpu()
    d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height, matrix, range)
    if where != _lib.VD_HOST:
        raise ValueError("yuv420_16_to_rgb() converts host frames")
    out = np.empty((n, max(h, 0), max(w, 0), 3), np.uint8)
    check(_lib.load().vd_yuv420_16_to_rgb(ctypes.byref(d), n, h, w, ptr(out), w * 3))
    del keep
    return out


def jpeg_info(data):
    """(h, w, components) of a baseline JPEG (host-only parse, no GPU). A bytes object is
    parsed in place (its own buffer: no copy -- a 2.4-MB frame copied under the GIL for every
    frame of a batch stalled the decode / process / encode threads of GpuJpegStages)."""
    lib = _lib.load()
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if isinstance(data, bytes):
        keep = ctypes.c_char_p(data)
        buf = ctypes.cast(keep, ctypes.c_void_p)
    else:
        buf = keep = ctypes.create_string_buffer(bytes(data), len(data))
    check(lib.vd_jpeg_info(buf, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)))
    del keep
    return h.value, w.value, c.value


class DeviceBoxes:
    """vd_boxes backed by torch device tensors (kernels write them directly)."""

    def __init__(self, n, cap, device):
        import torch
        self.n, self.cap = n, cap
        self.count = torch.zeros(n, dtype=torch.int32, device=device)
        self.xyxy = torch.zeros((n, cap, 4), dtype=torch.int32, device=device)
        self.xyxy_f = torch.zeros((n, cap, 4), dtype=torch.float32, device=device)
        self.score = torch.zeros((n, cap), dtype=torch.float32, device=device)
        self.label = torch.zeros((n, cap), dtype=torch.int32, device=device)

    def struct(self):
        return _lib.vd_boxes(self.cap, _lib.VD_DEVICE, self.count.data_ptr(), self.xyxy.data_ptr(),
                             self.xyxy_f.data_ptr(), self.score.data_ptr(), self.label.data_ptr())

    def view(self, start, n):
        """Frames [start, start + n) as a DeviceBoxes sharing this one's storage (a call
        writing it fills exactly those rows)."""
        if start < 0 or n < 0 or start + n > self.n:
            raise ValueError(f"rows [{start}, {start + n}) outside [0, {self.n})")
        v = DeviceBoxes.__new__(DeviceBoxes)
        v.n, v.cap = n, self.cap
        for k in ("count", "xyxy", "xyxy_f", "score", "label"):
            setattr(v, k, getattr(self, k)[start:start + n])
        return v


def _rows(boxes, start, n):
    """Frames [start, start + n) of caller lists, sharing their storage (None stays None)."""
    if boxes is None:
        return None
    if isinstance(boxes, DeviceBoxes):
        return boxes.view(start, n)
    v = _lib.HostBoxes.__new__(_lib.HostBoxes)
    v.n, v.cap = n, boxes.cap
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        setattr(v, k, getattr(boxes, k)[start:start + n])
    return v


def _host_concat(parts):
    """Library-allocated host lists of consecutive sub-batches as one HostBoxes."""
    out = _lib.HostBoxes(sum(p.n for p in parts), max(p.cap for p in parts))
    r = 0
    for p in parts:
        out.count[r:r + p.n] = p.count
        for k in ("xyxy", "xyxy_f", "score", "label"):
            getattr(out, k)[r:r + p.n, :p.cap] = getattr(p, k)
        r += p.n
    return out


BLUR_MODES = {"pixelate": _lib.VD_BLUR_PIXELATE, "gaussian": _lib.VD_BLUR_GAUSSIAN}


class Context:
    """vd_create/vd_destroy with the reference-facing knobs as keyword args."""

    def __init__(self, device=0, precision="bf16", max_batch=64, input_shape=(640, 640), confidence=0.5,
                 nms_iou=0.4, max_boxes=256, mosaic_level=8, plate_nc=1, plate_conf=0.5, plate_iou=0.7,
                 plate_max_det=300, plate_imgsz=640, microbatch=0, microbatch_stage=2, options=None,
                 blur="pixelate", blur_ksize=31, blur_sigma=0.0, hold=0, hold_iou_pct=30,
                 hold_motion=False, mask="rect", mask_grow=0, tiles=(1, 1), tile_overlap=20, cells=0,
                 lead=0, lead_motion=False, rescue=0.0, plate_rescue=0.0, rescue_span=60, tile_nets="faces",
                 tile_surfaces=False, rescue_tiles=False):
        """blur: what process() applies to the kept boxes: "pixelate" (the reference's
        INTER_NEAREST mosaic, the default) or "gaussian" (GaussianBlur(region, (blur_ksize,
        blur_ksize), blur_sigma) per clipped box, in list order; blur_ksize odd in [3, 127],
        blur_sigma <= 0: cv2's rule from the kernel size).
        hold: box hold (include/vdmi.h): the context's calls are one stream of consecutive
        frames, and a box stays in process()'s blur list for up to `hold` frames (0 = off,
        at most 8) after the last frame in which a box matched it (100 * inter >=
        hold_iou_pct * union on the clipped boxes), so a missed detection never shows a
        face in the clear; hold_reset() starts a new stream.
        hold_motion (needs hold > 0): a held box is stretched along the displacement between
        its last two sightings (vd_hold_motion's linear mode): the hull of the stored box and
        its extrapolation `age` frames on, so it also covers a face that keeps moving. Same
        membership, order and ages; frames of at most 32768 x 32768. Kept as self.hold_motion
        (it is no vd_cfg field); set_hold_motion() changes it.
        mask / mask_grow: mask shaping (include/vdmi.h at vd_mask) of every list the context
        blurs (process(), mosaic(), blur()): each box grown by mask_grow percent (0..200; a side
        becomes about 1 + mask_grow/100 times as long) and, with mask="ellipse", only the
        ellipse inscribed in the grown box hidden (with mask_grow >= 42 that still covers every
        pixel of the box as detected). The default ("rect", 0) blurs the detector's rectangle.
        Kept as self.mask / self.mask_grow (no vd_cfg fields); set_mask() changes them.
        tiles / tile_overlap: tiled face detection (include/vdmi.h at vd_tiles): with tiles=(R, C),
        R * C > 1, every frame goes through the face net as the whole frame plus R x C crops at
        their native scale that overlap by tile_overlap percent, and the lists are merged by one
        more NMS, so faces too small for the letterboxed frame are still found. T = 1 + R * C net
        inputs per frame: a call carries max_batch // T frames, and detect() / process() split a
        longer batch. (1, 1) (the default) is off. Kept as self.tiles / self.tile_overlap;
        set_tiles() changes them.
        tile_nets: which nets the tiling applies to (include/vdmi.h at vd_tiles_nets): "faces" (the
        default: the plate net sees the whole frame only, as in an untiled context), "plates" (the
        plate net alone: small plates in high-resolution frames, at a fraction of the face net's
        cost) or "both". A tiled plate net gives T lists per frame, merged per class at plate_iou;
        the calls that run it carry max_batch // T frames and split a longer batch. No effect
        while tiles == (1, 1). Kept as self.tile_nets; set_tile_nets() changes it.
        tile_surfaces: whether the 4:2:0 surface calls (process_nv12 / process_yuv420 /
        process_yuv420_16 and their process_lead_* forms) run the tiled nets (include/vdmi.h at
        vd_tiles_surfaces). False (the default): they refuse a call that would run a tiled net, as
        they always did. True: every list equals the RGB tiled call's on the converted frames, and a
        long batch is split into consecutive calls of frames_per_call() frames as process() splits
        it. Kept as self.tile_surfaces; set_tile_surfaces() changes it.
        cells: box-scaled strength (include/vdmi.h at vd_cells): with cells = N in 2..64 every box
        is hidden with at most N cells along its longer side instead of a constant number of
        pixels -- pixelation picks its level per box (never below mosaic_level), and a
        "gaussian" context applies the scaled smooth blur (cell means interpolated across the
        box) in place of the fixed kernel, in process() and mosaic(); blur() stays the
        fixed-kernel Gaussian. 0 (the default) is off. Kept as self.cells; set_cells() changes it.
        lead / lead_motion: look-ahead hold (include/vdmi.h at vd_lead): a box first seen in one
        of the next `lead` frames (0 = off, at most 8) and matched by nothing before is already
        blurred, so a face never shows in the clear because its first detection came late. The
        definition is the box hold of the time-reversed stream under hold_iou_pct; lead_motion
        stretches a led box backwards along the way the face came. Such a context blurs through
        process_lead(), whose output lags its input by lead (+ 1 with lead_motion) frames, and
        must be flushed at the end of a stream (lead_flush()); process() with the mosaic flag
        is refused. Kept as self.lead / self.lead_motion (no vd_cfg fields); set_lead() changes
        them.
        rescue / plate_rescue / rescue_span: weak-detection rescue (include/vdmi.h at vd_rescue): a
        face box scored in [rescue, confidence) (a plate box in (plate_rescue, plate_conf]) that
        matches, under hold_iou_pct, a box blurred in one of the last max(1, hold) frames is blurred
        too, for at most rescue_span frames (1..255; the default 60 is one second at the
        reference's output rate) after the track's last strong detection. The detections that
        process() returns stay the strong ones. 0.0 / 0.0 (the default) is off. With tiles only
        under rescue_tiles. Kept as self.rescue_low / self.plate_rescue_low / self.rescue_span;
        rescue() changes them.
        rescue_tiles: whether rescue and tiling may be combined (include/vdmi.h at vd_rescue_tiles).
        False (the default): rescue() in a tiling context and set_tiles() in a rescue context are
        refused, as they always were. True: a tiled net's per-input lists run at the low threshold
        and the cross-tile merge makes the split, so the detections stay bit for bit those of the
        tiled context without rescue, and the weak boxes of the merged list take part in the rescue
        like an untiled net's. Applied before tiles and rescue. Kept as self.rescue_tiles;
        set_rescue_tiles() changes it."""
        if blur not in BLUR_MODES:
            raise ValueError(f"blur {blur!r}: expected 'pixelate' or 'gaussian'")
        hold, hold_iou_pct = _lib.check_hold(hold, hold_iou_pct, hold_motion)   # before the library is touched
        mask, mask_grow = _lib.check_mask(mask, mask_grow)
        tiles, tile_overlap = _lib.check_tiles(tiles, tile_overlap)
        tile_nets = _lib.check_tile_nets(tile_nets)
        tile_surfaces = _lib.check_tile_surfaces(tile_surfaces)
        rescue_tiles = _lib.check_rescue_tiles(rescue_tiles)
        cells = _lib.check_cells(cells)
        lead, lead_motion = _lib.check_lead(lead, lead_motion)
        rescue, plate_rescue, rescue_span = _lib.check_rescue(rescue, plate_rescue, rescue_span)
        lib = _lib.load()
        cfg = _lib.default_cfg()
        cfg.input_h, cfg.input_w = int(input_shape[0]), int(input_shape[1])
        cfg.max_batch = int(max_batch)
        if precision in ("fp32", "f32", "float32"):
            cfg.precision = _lib.VD_PREC_FP32
        elif precision in ("fp16", "f16", "float16", "half"):
            cfg.precision = _lib.VD_PREC_FP16
        elif precision in ("bf16", "bfloat16"):
            cfg.precision = _lib.VD_PREC_BF16
        else:
            raise ValueError(f"precision {precision!r}: expected 'bf16', 'fp16' or 'fp32'")
        cfg.confidence = float(confidence)
        cfg.nms_iou = float(nms_iou)
        cfg.max_boxes = int(max_boxes)
        cfg.mosaic_level = int(mosaic_level)
        cfg.plate_nc, cfg.plate_conf, cfg.plate_iou = int(plate_nc), float(plate_conf), float(plate_iou)
        cfg.plate_max_det, cfg.plate_imgsz = int(plate_max_det), int(plate_imgsz)
        # depth-first micro-batching of the backbone through layer<stage>
        cfg.microbatch, cfg.microbatch_stage = int(microbatch), int(microbatch_stage)
        cfg.blur_mode = BLUR_MODES[blur]
        if cfg.blur_mode == _lib.VD_BLUR_GAUSSIAN:      # pixelate leaves the fields zero
            cfg.blur_ksize, cfg.blur_sigma = int(blur_ksize), float(blur_sigma)
        if hold:                                        # off leaves the fields zero
            cfg.hold_frames, cfg.hold_iou_pct = hold, hold_iou_pct
        elif lead or rescue or plate_rescue:            # the lead / rescue match uses the same threshold
            cfg.hold_iou_pct = hold_iou_pct
        self.cfg = cfg
        self.device = int(device)
        self.precision = {_lib.VD_PREC_FP32: "fp32", _lib.VD_PREC_FP16: "fp16"}.get(cfg.precision, "bf16")
        h = ctypes.c_void_p()
        check(lib.vd_create(ctypes.byref(cfg), self.device, ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self.hold_motion = False
        if hold_motion:
            self.set_hold_motion(True)
        self.mask, self.mask_grow = "rect", 0
        if (mask, mask_grow) != ("rect", 0):
            self.set_mask(mask, mask_grow)
        self.rescue_tiles = False
        if rescue_tiles:                                # before tiles and rescue: it lets them combine
            self.set_rescue_tiles(True)
        self.tiles, self.tile_overlap = (1, 1), tile_overlap
        if tiles != (1, 1):
            self.set_tiles(tiles, tile_overlap)
        self.tile_nets = "faces"
        if tile_nets != "faces":
            self.set_tile_nets(tile_nets)
        self.tile_surfaces = False
        if tile_surfaces:
            self.set_tile_surfaces(True)
        self.cells = 0
        if cells:
            self.set_cells(cells)
        self.lead, self.lead_motion = 0, False
        if lead:
            self.set_lead(lead, lead_motion)
        self.rescue_low, self.plate_rescue_low, self.rescue_span = 0.0, 0.0, rescue_span
        if rescue or plate_rescue:
            self.rescue(rescue, plate_rescue, rescue_span)
        for k, v in dict(options or {}).items():   # kernel-selection switches (vd_set_option)
            self.set_option(k, v)

    # -- lifecycle -------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.vd_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def load_weights(self, net, state_dict_or_blob):
        from .weights import pack_vdw
        blob = state_dict_or_blob if isinstance(state_dict_or_blob, (bytes, bytearray)) else pack_vdw(state_dict_or_blob)
        buf = ctypes.create_string_buffer(bytes(blob), len(blob))
        check(self._lib.vd_load_weights(self._h, net, buf, len(blob), _lib.VD_WEIGHTS_VDW1))

    def set_option(self, name, value):
        check(self._lib.vd_set_option(self._h, str(name).encode(), int(value)))

    def set_debug(self, name, value):
        """Timing-only experiment switches (vdt_set_debug: "x6_dbg", "block32_dbg"); the
        results are WRONG while they are set. Never a production knob."""
        check(self._lib.vdt_set_debug(self._h, str(name).encode(), int(value)))

    def set_stream(self, stream_ptr):
        check(self._lib.vd_set_stream(self._h, stream_ptr))

    def stream(self):
        return self._lib.vd_get_stream(self._h)

    def stream_wait_event(self, event):
        """Queue a wait for a torch.cuda.Event on this context's stream (orders its next
        launches behind work recorded on another context's or torch's stream)."""
        import torch
        torch.cuda.ExternalStream(self.stream(), device=torch.device(f"cuda:{self.device}")).wait_event(event)

    def sync(self):
        check(self._lib.vd_sync(self._h))

    # -- hot path ----------------------------------------------------------
    def _boxes(self, boxes, n):
        if boxes is None:
            boxes = _lib.HostBoxes(n, self.cfg.max_boxes)
        return boxes

    def read_boxes(self, net, n, cap=None):
        """The complete keep lists of the last call for frames [0, n) (vd_read_boxes) as
        HostBoxes; cap defaults to the largest count."""
        if cap is None:
            cnt = _lib.HostBoxes(n, 1)
            check(self._lib.vd_read_boxes(self._h, net, n, ctypes.byref(cnt.struct())))
            cap = max(1, int(cnt.count.max()))
        boxes = _lib.HostBoxes(n, cap)
        check(self._lib.vd_read_boxes(self._h, net, n, ctypes.byref(boxes.struct())))
        return boxes

    def _complete(self, boxes, net, auto):
        """Library-allocated host lists never come back truncated: a frame that kept
        more than cfg.max_boxes boxes triggers a re-read of the complete lists."""
        if auto and isinstance(boxes, _lib.HostBoxes) and boxes.n and int(boxes.count.max()) > boxes.cap:
            return self.read_boxes(net, boxes.n, int(boxes.count.max()))
        return boxes

    def detect(self, frames, boxes=None):
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        step = self.frames_per_call(faces=True, plates=False)
        if n > step and step < self.cfg.max_batch:     # tiling: max_batch // T frames per call
            parts = [self.detect(keep[s0:s0 + step], _rows(boxes, s0, min(step, n - s0)))
                     for s0 in range(0, n, step)]
            return boxes if boxes is not None else _host_concat(parts)
        auto = boxes is None
        boxes = self._boxes(boxes, n)
        s = boxes.struct()
        check(self._lib.vd_detect(self._h, p, n, h, w, pitch, where, ctypes.byref(s)))
        return self._complete(boxes, _lib.VD_NET_RETINAFACE, auto)

    def frames_per_call(self, faces=True, plates=True):
        """Frames one call carries: max_batch, or max_batch // T when it runs a tiled net. faces /
        plates: the nets the call runs (by default both: the bound that holds for every call)."""
        r, c = self.tiles
        nets = _lib.TILE_NETS[self.tile_nets]
        tiled = r * c > 1 and ((faces and nets & _lib.VD_TILE_FACES) or (plates and nets & _lib.VD_TILE_PLATES))
        return max(1, self.cfg.max_batch // (1 + r * c)) if tiled else self.cfg.max_batch

    def _step(self, flags):
        """frames_per_call() of a process() / process_lead() call with these flags."""
        return self.frames_per_call(bool(flags & _lib.VD_PROC_FACES), bool(flags & _lib.VD_PROC_PLATES))

    def detect_plates(self, frames, boxes=None):
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        step = self.frames_per_call(faces=False, plates=True)
        if n > step and step < self.cfg.max_batch:     # plates tiled: max_batch // T frames per call
            parts = [self.detect_plates(keep[s0:s0 + step], _rows(boxes, s0, min(step, n - s0)))
                     for s0 in range(0, n, step)]
            return boxes if boxes is not None else _host_concat(parts)
        auto = boxes is None
        boxes = self._boxes(boxes, n)
        s = boxes.struct()
        check(self._lib.vd_detect_plates(self._h, p, n, h, w, pitch, where, ctypes.byref(s)))
        return self._complete(boxes, _lib.VD_NET_YOLOV8N, auto)

    def _blur_args(self, frames, boxes_xyxy, counts, out, pitched):
        """What mosaic() / blur() / smooth() share -> (the C call's arguments from `in` to `boxes`,
        out, keepalive). boxes_xyxy: int32 [n][cap][4] (host numpy) with counts int32 [n], or a
        HostBoxes / DeviceBoxes. pitched: a torch view with padded rows (big[:, :, :w]) is read
        and written at its own row pitch, and a torch `out` must have the frames' layout."""
        p, n, h, w, pitch, where, src = _frames_arg(frames, pitched=pitched)
        if isinstance(boxes_xyxy, (_lib.HostBoxes, DeviceBoxes)):
            s = boxes_xyxy.struct()
            keep = (src, s)
        else:
            xy = np.ascontiguousarray(boxes_xyxy, np.int32).reshape(n, -1, 4)
            cnt = np.ascontiguousarray(counts if counts is not None else np.full(n, xy.shape[1]), np.int32)
            cap = max(1, xy.shape[1])
            if xy.shape[1] == 0:
                xy = np.zeros((n, 1, 4), np.int32)
            s = _lib.vd_boxes(cap, _lib.VD_HOST, ptr(cnt), ptr(xy), None, None, None)
            keep = (src, s, xy, cnt)
        if out is None:
            if pitch != w * 3:
                raise ValueError("frames with padded rows need out= (a view with the same row pitch)")
            if where == _lib.VD_HOST:
                out = np.empty((n, h, w, 3), np.uint8)
            else:
                import torch
                out = torch.empty_like(src if pitched else frames)
        if pitched and _is_torch(out):
            packed = out.is_contiguous()
            if tuple(out.shape) != (n, h, w, 3) or not (packed or _row_padded(out)) or \
                    (w * 3 if packed else out.stride(1)) != pitch:
                raise ValueError("out must be uint8 [n,h,w,3] with the frames' row pitch")
        optr = out.data_ptr() if _is_torch(out) else ptr(out)
        return (p, optr, n, h, w, pitch, where, ctypes.byref(s)), out, keep

    def mosaic(self, frames, boxes_xyxy, counts=None, level=None, out=None):
        """Out-of-place mosaic. boxes_xyxy: int32 [n][cap][4] (host numpy) or a
        HostBoxes/DeviceBoxes; counts: int32 [n] (host) when boxes_xyxy is an array."""
        args, out, keep = self._blur_args(frames, boxes_xyxy, counts, out, pitched=False)
        check(self._lib.vd_mosaic(self._h, *args, int(level or self.cfg.mosaic_level), _lib.VD_MOSAIC_OUT_OF_PLACE))
        return out

    def blur(self, frames, boxes_xyxy, counts=None, ksize=None, sigma=None, out=None):
        """Out-of-place Gaussian blur of the boxes (vd_blur), the counterpart of mosaic():
        the same frames / boxes_xyxy / counts forms. ksize / sigma default to the context's
        blur_ksize / blur_sigma (31 / 0 in a pixelate context). A torch view with padded
        rows (big[:, :, :w]) is read and written at its own row pitch."""
        args, out, keep = self._blur_args(frames, boxes_xyxy, counts, out, pitched=True)
        if ksize is None:
            ksize = self.cfg.blur_ksize or 31
        if sigma is None:
            sigma = self.cfg.blur_sigma
        check(self._lib.vd_blur(self._h, *args, int(ksize), float(sigma)))
        return out

    def smooth(self, frames, boxes_xyxy, counts=None, level=None, cells=None, out=None):
        """Out-of-place scaled smooth blur of the boxes (vd_smooth), the counterpart of mosaic()
        and blur(): the same frames / boxes_xyxy / counts forms, a torch view with padded rows
        (big[:, :, :w]) read and written at its own row pitch. level defaults to the context's
        mosaic_level, cells to the context's setting (ValueError if that is 0: off)."""
        cells = _lib.check_cells(self.cells if cells is None else cells)
        if cells == 0:
            raise ValueError("smooth() needs cells in 2 .. 64 (the context's setting is 0: off)")
        args, out, keep = self._blur_args(frames, boxes_xyxy, counts, out, pitched=True)
        check(self._lib.vd_smooth(self._h, *args, int(level or self.cfg.mosaic_level), cells))
        return out

    def process(self, frames, out=None, faces=None, plates=None, flags=None):
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        if out is None and flags & _lib.VD_PROC_MOSAIC:
            if where == _lib.VD_HOST:
                out = np.empty((n, h, w, 3), np.uint8)
            else:
                import torch
                out = torch.empty_like(frames)
        step = self._step(flags)
        if n > step and step < self.cfg.max_batch:     # a tiled net: consecutive calls (exact under hold:
            pf, pp = [], []                            # the history carries across calls)
            for s0 in range(0, n, step):
                k = min(step, n - s0)
                _, f, q = self.process(keep[s0:s0 + k], None if out is None else out[s0:s0 + k],
                                       _rows(faces, s0, k), _rows(plates, s0, k), flags)
                pf.append(f)
                pp.append(q)
            if faces is None:
                faces = _host_concat(pf)
            if plates is None and flags & _lib.VD_PROC_PLATES:
                plates = _host_concat(pp)
            return out, faces, plates
        fs = ps = None
        auto_f, auto_p = faces is None, plates is None
        if flags & _lib.VD_PROC_FACES:
            faces = self._boxes(faces, n)
            fs = faces.struct()
        if flags & _lib.VD_PROC_PLATES:
            plates = self._boxes(plates, n)
            ps = plates.struct()
        optr = None if out is None else (out.data_ptr() if _is_torch(out) else ptr(out))
        check(self._lib.vd_process(self._h, p, optr, n, h, w, pitch, where, flags,
                                   ctypes.byref(fs) if fs is not None else None,
                                   ctypes.byref(ps) if ps is not None else None))
        if flags & _lib.VD_PROC_FACES:
            faces = self._complete(faces, _lib.VD_NET_RETINAFACE, auto_f)
        if flags & _lib.VD_PROC_PLATES:
            plates = self._complete(plates, _lib.VD_NET_YOLOV8N, auto_p)
        return out, faces, plates

    # -- 4:2:0 surfaces: what the process_* calls of every descriptor family share -------
    @staticmethod
    def _from_frame(d, s0):
        """The descriptor of frames s0, s0 + 1, ... of the batch d describes (None stays None)."""
        if d is None or s0 == 0:
            return d
        e = type(d).from_buffer_copy(d)
        e.base = d.base + s0 * d.frame_stride
        return e

    def _surface_step(self, flags):
        """Frames one surface call carries: frames_per_call() where tile_surfaces lets it run a tiled net."""
        return self._step(flags) if self.tile_surfaces else self.cfg.max_batch

    def _process_420(self, fn, d, od, n, h, w, where, flags, faces, plates):
        """fn = vd_process_nv12 / _yuv420 / _yuv420_16 on checked descriptors -> (faces, plates). A tiled
        net: consecutive calls of frames_per_call() frames, as process() (exact under hold: the history
        carries across calls)."""
        step = self._surface_step(flags)
        if n > step and step < self.cfg.max_batch:
            pf, pp = [], []
            for s0 in range(0, n, step):
                k = min(step, n - s0)
                f, q = self._process_420(fn, self._from_frame(d, s0), self._from_frame(od, s0), k, h, w, where, flags,
                                         _rows(faces, s0, k), _rows(plates, s0, k))
                pf.append(f)
                pp.append(q)
            if faces is None:
                faces = _host_concat(pf)
            if plates is None and flags & _lib.VD_PROC_PLATES:
                plates = _host_concat(pp)
            return faces, plates
        fs = ps = None
        auto_f, auto_p = faces is None, plates is None
        if flags & _lib.VD_PROC_FACES:
            faces = self._boxes(faces, n)
            fs = faces.struct()
        if flags & _lib.VD_PROC_PLATES:
            plates = self._boxes(plates, n)
            ps = plates.struct()
        check(fn(self._h, ctypes.byref(d), ctypes.byref(od) if od is not None else None, n, h, w, where, flags,
                 ctypes.byref(fs) if fs is not None else None, ctypes.byref(ps) if ps is not None else None))
        if flags & _lib.VD_PROC_FACES:
            faces = self._complete(faces, _lib.VD_NET_RETINAFACE, auto_f)
        if flags & _lib.VD_PROC_PLATES:
            plates = self._complete(plates, _lib.VD_NET_YOLOV8N, auto_p)
        return faces, plates

    def _lead_calls_420(self, fn, d, od, cap, n, h, w, where, flags, faces, plates, flush):
        """fn = vd_process_lead_nv12 / _yuv420 / _yuv420_16 on checked descriptors (od: room for cap
        surfaces, None when cap is 0) -> (m, faces, plates). A tiled net: consecutive calls as
        _process_420's, what they emit written one after the other; only the last one flushes."""
        step = self._surface_step(flags)
        if n > step and step < self.cfg.max_batch:
            pf, pp, m = [], [], 0
            for s0 in range(0, n, step):
                k = min(step, n - s0)
                mk, f, q = self._lead_calls_420(fn, self._from_frame(d, s0), self._from_frame(od, m) if cap > m else None,
                                                cap - m, k, h, w, where, flags, _rows(faces, s0, k), _rows(plates, s0, k),
                                                flush and s0 + k == n)
                m += mk
                pf.append(f)
                pp.append(q)
            if faces is None:
                faces = _host_concat(pf)
            if plates is None and flags & _lib.VD_PROC_PLATES:
                plates = _host_concat(pp)
            return m, faces, plates
        fs = ps = None
        auto_f, auto_p = faces is None, plates is None
        if flags & _lib.VD_PROC_FACES:
            faces = self._boxes(faces, n)
            fs = faces.struct()
        if flags & _lib.VD_PROC_PLATES:
            plates = self._boxes(plates, n)
            ps = plates.struct()
        m = ctypes.c_int(0)
        check(fn(self._h, ctypes.byref(d), ctypes.byref(od) if od is not None else None, n, h, w, where, flags,
                 ctypes.byref(fs) if fs is not None else None, ctypes.byref(ps) if ps is not None else None, cap,
                 1 if flush else 0, ctypes.byref(m)))
        if flags & _lib.VD_PROC_FACES:
            faces = self._complete(faces, _lib.VD_NET_RETINAFACE, auto_f)
        if flags & _lib.VD_PROC_PLATES:
            plates = self._complete(plates, _lib.VD_NET_YOLOV8N, auto_p)
        return m.value, faces, plates

    # -- NV12 frames ---------------------------------------------------------------
    @staticmethod
    def _nv12_out(frames, out, height):
        """The output surfaces of an NV12 blurring call: `out` in any layout of _nv12_arg, or new
        ones like the input -> (out, vd_nv12, keepalive)."""
        if out is None:
            if _is_torch(frames):
                import torch
                out = torch.empty_like(frames, memory_format=torch.contiguous_format)
            else:
                out = np.empty(np.shape(frames), np.uint8)
        d, n, h, w, where, keep = _nv12_arg(out, height, writable=True)
        return out, d, (n, h, w, where), keep

    def process_nv12(self, frames, out=None, faces=None, plates=None, flags=None, matrix="bt709", range="limited",
                     height=None):
        """vd_process_nv12: process() on NV12 frames (uint8 [n, rows, w]; _nv12_arg gives the
        layouts). Detections are exactly process()'s on nv12_to_rgb(frames); with VD_PROC_MOSAIC
        both planes of `out` (default: new surfaces like the input) are blurred as the context's
        settings ask: pixelation, or with blur="gaussian" and cells on the scaled smooth blur, under
        the mask setting (blur="gaussian" with cells=0 has no NV12 pass). In a tiling context the call
        is refused unless tile_surfaces is on; then the lists are process()'s of the tiled context on
        nv12_to_rgb(frames) and a long batch is split as process() splits it. -> (out, faces, plates)."""
        d, n, h, w, where, keep = _nv12_arg(frames, height, matrix, range)
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        od = None
        if flags & _lib.VD_PROC_MOSAIC:
            out, od, geo, okeep = self._nv12_out(frames, out, height)
            if geo != (n, h, w, where):
                raise ValueError("out must hold NV12 frames of the input's n, h, w in the same memory (host / device)")
        faces, plates = self._process_420(self._lib.vd_process_nv12, d, od, n, h, w, where, flags, faces, plates)
        del keep
        return out, faces, plates

    def _nv12_blur(self, fn, frames, boxes_xyxy, counts, out, height, *tail):
        """What mosaic_nv12() / smooth_nv12() share: fn(ctx, in, out, n, h, w, where, boxes, *tail)."""
        d, n, h, w, where, keep = _nv12_arg(frames, height)
        if isinstance(boxes_xyxy, (_lib.HostBoxes, DeviceBoxes)):
            s = boxes_xyxy.struct()
            bkeep = None
        else:
            xy = np.ascontiguousarray(boxes_xyxy, np.int32).reshape(n, -1, 4)
            cnt = np.ascontiguousarray(counts if counts is not None else np.full(n, xy.shape[1]), np.int32)
            cap = max(1, xy.shape[1])
            if xy.shape[1] == 0:
                xy = np.zeros((n, 1, 4), np.int32)
            s = _lib.vd_boxes(cap, _lib.VD_HOST, ptr(cnt), ptr(xy), None, None, None)
            bkeep = (xy, cnt)
        out, od, geo, okeep = self._nv12_out(frames, out, height)
        if geo != (n, h, w, where):
            raise ValueError("out must hold NV12 frames of the input's n, h, w in the same memory (host / device)")
        check(fn(self._h, ctypes.byref(d), ctypes.byref(od), n, h, w, where, ctypes.byref(s), *tail))
        del keep, bkeep, okeep
        return out

    def mosaic_nv12(self, frames, boxes_xyxy, counts=None, level=None, out=None, height=None):
        """vd_mosaic_nv12: the out-of-place blur of both planes of NV12 frames with caller lists (the
        boxes_xyxy / counts forms of mosaic()) that the context's blur mode asks for: pixelation, or
        in a blur="gaussian" context with cells on the scaled smooth blur. The context's mask
        setting and cells apply."""
        return self._nv12_blur(self._lib.vd_mosaic_nv12, frames, boxes_xyxy, counts, out, height,
                               int(level or self.cfg.mosaic_level))

    def smooth_nv12(self, frames, boxes_xyxy, counts=None, level=None, cells=None, out=None, height=None):
        """vd_smooth_nv12: the out-of-place scaled smooth blur of both planes of NV12 frames with
        caller lists, the counterpart of smooth(). level defaults to the context's mosaic_level,
        cells to the context's setting (ValueError if that is 0: off); the mask setting applies."""
        cells = _lib.check_cells(self.cells if cells is None else cells)
        if cells == 0:
            raise ValueError("smooth_nv12() needs cells in 2 .. 64 (the context's setting is 0: off)")
        return self._nv12_blur(self._lib.vd_smooth_nv12, frames, boxes_xyxy, counts, out, height,
                               int(level or self.cfg.mosaic_level), cells)

    def letterbox_nv12(self, frames, cpad=4, matrix="bt709", range="limited", height=None):
        """vdt_letterbox_nv12: the face canvas of NV12 frames by the product path's NV12 kernel."""
        d, n, h, w, where, keep = _nv12_arg(frames, height, matrix, range)
        out = np.zeros((n, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(self._lib.vdt_letterbox_nv12(self._h, ctypes.byref(d), n, h, w, where, ptr(out), cpad))
        del keep
        return out

    # -- 4:2:0 frames in any layout (I420, YV12, NV12, NV21) ------------------------------
    @staticmethod
    def _yuv420_out(frames, geo, out, out_layout, height):
        """The output surfaces of a 4:2:0 blurring call: `out` (an array in out_layout, or a Yuv420),
        or new packed frames [n, 3h/2, w] in out_layout where the input lives -> (out, vd_yuv420, geo, keep)."""
        n, h, w, where = geo
        if out is None:
            src = frames.buffer if isinstance(frames, Yuv420) else frames
            if _is_torch(src):
                import torch
                out = torch.empty((n, h // 2 * 3, w), dtype=torch.uint8, device=src.device)
            else:
                out = np.empty((n, h // 2 * 3, w), np.uint8)
            height = None
        d, on, oh, ow, owhere, keep = _yuv420_arg(out, out_layout, height, writable=True)
        return out, d, (on, oh, ow, owhere), keep

    def process_yuv420(self, frames, out=None, faces=None, plates=None, flags=None, layout="i420", out_layout=None,
                       matrix="bt709", range="limited", height=None):
        """vd_process_yuv420: process_nv12() on 8-bit 4:2:0 frames in any layout -- layout / out_layout
        in "i420", "yv12", "nv12", "nv21" (out_layout defaults to layout), frames uint8 [n, 3h/2, w]
        (_yuv420_arg) or a Yuv420. Lists are exactly process_nv12()'s on the NV12 frames with the same
        samples, and so is every sample of `out`; in and out layouts may differ. max_batch, hold,
        rescue, mask and cells act as in process_nv12(). -> (out, faces, plates)."""
        d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        od = None
        if flags & _lib.VD_PROC_MOSAIC:
            out, od, geo, okeep = self._yuv420_out(frames, (n, h, w, where), out, out_layout or layout, height)
            if geo != (n, h, w, where):
                raise ValueError("out must hold 4:2:0 frames of the input's n, h, w in the same memory (host / device)")
        faces, plates = self._process_420(self._lib.vd_process_yuv420, d, od, n, h, w, where, flags, faces, plates)
        del keep
        return out, faces, plates

    def _yuv420_blur(self, fn, frames, boxes_xyxy, counts, out, layout, out_layout, height, *tail):
        """What mosaic_yuv420() / smooth_yuv420() share: fn(ctx, in, out, n, h, w, where, boxes, *tail)."""
        d, n, h, w, where, keep = _yuv420_arg(frames, layout, height)
        if isinstance(boxes_xyxy, (_lib.HostBoxes, DeviceBoxes)):
            s = boxes_xyxy.struct()
            bkeep = None
        else:
            xy = np.ascontiguousarray(boxes_xyxy, np.int32).reshape(n, -1, 4)
            cnt = np.ascontiguousarray(counts if counts is not None else np.full(n, xy.shape[1]), np.int32)
            cap = max(1, xy.shape[1])
            if xy.shape[1] == 0:
                xy = np.zeros((n, 1, 4), np.int32)
            s = _lib.vd_boxes(cap, _lib.VD_HOST, ptr(cnt), ptr(xy), None, None, None)
            bkeep = (xy, cnt)
        out, od, geo, okeep = self._yuv420_out(frames, (n, h, w, where), out, out_layout or layout, height)
        if geo != (n, h, w, where):
            raise ValueError("out must hold 4:2:0 frames of the input's n, h, w in the same memory (host / device)")
        check(fn(self._h, ctypes.byref(d), ctypes.byref(od), n, h, w, where, ctypes.byref(s), *tail))
        del keep, bkeep, okeep
        return out

    def mosaic_yuv420(self, frames, boxes_xyxy, counts=None, level=None, out=None, layout="i420", out_layout=None,
                      height=None):
        """vd_mosaic_yuv420: mosaic_nv12() on 4:2:0 frames in any layout, in and out layouts independent."""
        return self._yuv420_blur(self._lib.vd_mosaic_yuv420, frames, boxes_xyxy, counts, out, layout, out_layout, height,
                                 int(level or self.cfg.mosaic_level))

    def smooth_yuv420(self, frames, boxes_xyxy, counts=None, level=None, cells=None, out=None, layout="i420",
                      out_layout=None, height=None):
        """vd_smooth_yuv420: smooth_nv12() on 4:2:0 frames in any layout, in and out layouts independent."""
        cells = _lib.check_cells(self.cells if cells is None else cells)
        if cells == 0:
            raise ValueError("smooth_yuv420() needs cells in 2 .. 64 (the context's setting is 0: off)")
        return self._yuv420_blur(self._lib.vd_smooth_yuv420, frames, boxes_xyxy, counts, out, layout, out_layout, height,
                                 int(level or self.cfg.mosaic_level), cells)

    def letterbox_yuv420(self, frames, cpad=4, layout="i420", matrix="bt709", range="limited", height=None):
        """vdt_letterbox_yuv420: the face canvas of 4:2:0 frames by the product path's kernel for the layout."""
        d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
        out = np.zeros((n, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(self._lib.vdt_letterbox_yuv420(self._h, ctypes.byref(d), n, h, w, where, ptr(out), cpad))
        del keep
        return out

    # -- 10- and 12-bit 4:2:0 frames (P010, P012, yuv420p10le, yuv420p12le) ---------------
    @staticmethod
    def _yuv420_16_out(frames, geo, out, out_layout, depth, shift, height):
        """The output surfaces of a 16-bit 4:2:0 blurring call: `out` (a uint16 array in out_layout, or a
        Yuv420_16), or new packed frames [n, 3h/2, w] in out_layout where the input lives, in the input's
        depth and shift -> (out, vd_yuv420_16, geo, keep)."""
        n, h, w, where = geo
        if out is None:
            src = frames.buffer if isinstance(frames, Yuv420_16) else frames
            if _is_torch(src):
                import torch
                out = torch.empty((n, h // 2 * 3, w), dtype=torch.int16, device=src.device)
            else:
                out = np.empty((n, h // 2 * 3, w), np.uint16)
            height = None
        d, on, oh, ow, owhere, keep = _yuv420_16_arg(out, out_layout, depth, shift, height, writable=True)
        return out, d, (on, oh, ow, owhere), keep

    def process_yuv420_16(self, frames, out=None, faces=None, plates=None, flags=None, layout="i420", out_layout=None,
                          depth=10, shift=None, matrix="bt709", range="limited", height=None):
        """vd_process_yuv420_16: process_yuv420() on 10- or 12-bit 4:2:0 frames -- uint16 [n, 3h/2, w] in
        `layout` (_yuv420_16_arg) or a Yuv420_16. Lists are exactly process_yuv420()'s on the 8-bit
        picture of the frames (each value >> (depth - 8)); the blur acts on the 16-bit samples and every
        word outside a hidden box comes back as it was. out keeps the input's depth and shift (an array:
        those given here; a Yuv420_16: its own, which must match). -> (out, faces, plates)."""
        d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height, matrix, range)
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        od = None
        if flags & _lib.VD_PROC_MOSAIC:
            out, od, geo, okeep = self._yuv420_16_out(frames, (n, h, w, where), out, out_layout or layout, d.depth, d.shift,
                                                      height)
            if geo != (n, h, w, where):
                raise ValueError("out must hold 4:2:0 frames of the input's n, h, w in the same memory (host / device)")
        faces, plates = self._process_420(self._lib.vd_process_yuv420_16, d, od, n, h, w, where, flags, faces, plates)
        del keep
        return out, faces, plates

    def _yuv420_16_blur(self, fn, frames, boxes_xyxy, counts, out, layout, out_layout, depth, shift, height, *tail):
        """What mosaic_yuv420_16() / smooth_yuv420_16() share: fn(ctx, in, out, n, h, w, where, boxes, *tail)."""
        d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height)
        if isinstance(boxes_xyxy, (_lib.HostBoxes, DeviceBoxes)):
            s = boxes_xyxy.struct()
            bkeep = None
        else:
            xy = np.ascontiguousarray(boxes_xyxy, np.int32).reshape(n, -1, 4)
            cnt = np.ascontiguousarray(counts if counts is not None else np.full(n, xy.shape[1]), np.int32)
            cap = max(1, xy.shape[1])
            if xy.shape[1] == 0:
                xy = np.zeros((n, 1, 4), np.int32)
            s = _lib.vd_boxes(cap, _lib.VD_HOST, ptr(cnt), ptr(xy), None, None, None)
            bkeep = (xy, cnt)
        out, od, geo, okeep = self._yuv420_16_out(frames, (n, h, w, where), out, out_layout or layout, d.depth, d.shift, height)
        if geo != (n, h, w, where):
            raise ValueError("out must hold 4:2:0 frames of the input's n, h, w in the same memory (host / device)")
        check(fn(self._h, ctypes.byref(d), ctypes.byref(od), n, h, w, where, ctypes.byref(s), *tail))
        del keep, bkeep, okeep
        return out

    def mosaic_yuv420_16(self, frames, boxes_xyxy, counts=None, level=None, out=None, layout="i420", out_layout=None,
                         depth=10, shift=None, height=None):
        """vd_mosaic_yuv420_16: mosaic_yuv420() on 10- or 12-bit 4:2:0 frames; whole words are copied."""
        return self._yuv420_16_blur(self._lib.vd_mosaic_yuv420_16, frames, boxes_xyxy, counts, out, layout, out_layout,
                                    depth, shift, height, int(level or self.cfg.mosaic_level))

    def smooth_yuv420_16(self, frames, boxes_xyxy, counts=None, level=None, cells=None, out=None, layout="i420",
                         out_layout=None, depth=10, shift=None, height=None):
        """vd_smooth_yuv420_16: smooth_yuv420() on the values of 10- or 12-bit 4:2:0 frames."""
        cells = _lib.check_cells(self.cells if cells is None else cells)
        if cells == 0:
            raise ValueError("smooth_yuv420_16() needs cells in 2 .. 64 (the context's setting is 0: off)")
        return self._yuv420_16_blur(self._lib.vd_smooth_yuv420_16, frames, boxes_xyxy, counts, out, layout, out_layout,
                                    depth, shift, height, int(level or self.cfg.mosaic_level), cells)

    def letterbox_yuv420_16(self, frames, cpad=4, layout="i420", depth=10, shift=None, matrix="bt709", range="limited",
                            height=None):
        """vdt_letterbox_yuv420_16: the face canvas of 10- / 12-bit 4:2:0 frames by the product path's kernel."""
        d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height, matrix, range)
        out = np.zeros((n, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(self._lib.vdt_letterbox_yuv420_16(self._h, ctypes.byref(d), n, h, w, where, ptr(out), cpad))
        del keep
        return out

    # -- box hold ----------------------------------------------------------------
    def hold(self, boxes, h, w, out=None):
        """vd_hold: the hold step alone, for callers with their own detectors. boxes: the
        detections of consecutive h x w frames -- a HostBoxes / DeviceBoxes, or a list with
        one int [k][4] array per frame. Returns `out` (default: HostBoxes sized for the
        largest list) holding every frame's blur list, the frame's own boxes then the held
        ones, label = age (0: own; a: last seen a frames ago). The context's history is
        updated as by process()."""
        det = self._box_lists(boxes)
        n = det.n
        ds = det.struct()
        if out is not None:
            s = out.struct()
            check(self._lib.vd_hold(self._h, ctypes.byref(ds), n, int(h), int(w), ctypes.byref(s)))
            return out
        # sizes are not known before the step and the step must run once: take it without a
        # target, read the held boxes (complete), and put each frame's own boxes in front
        check(self._lib.vd_hold(self._h, ctypes.byref(ds), n, int(h), int(w), None))
        held = self.read_held(n)
        host = lambda t: t.cpu().numpy() if _is_torch(t) else t
        own = np.minimum(host(det.count), det.cap)
        xy = host(det.xyxy)
        out = _lib.HostBoxes(n, max(1, int((own + held.count).max())))
        for i in range(n):
            k, m = int(own[i]), int(held.count[i])
            out.count[i] = k + m
            out.xyxy[i, :k] = xy[i, :k]
            out.xyxy[i, k:k + m] = held.xyxy[i, :m]
            out.label[i, k:k + m] = held.label[i, :m]
        return out

    def hold_reset(self):
        """vd_hold_reset: forget the history; the next frame starts a new stream."""
        check(self._lib.vd_hold_reset(self._h))

    def set_hold_motion(self, on):
        """vd_hold_motion: held boxes follow the motion of their last two sightings (True) or
        stay where they were last seen (False). A change forgets the history."""
        mode = _lib.VD_HOLD_MOTION_LINEAR if on else _lib.VD_HOLD_MOTION_OFF
        check(self._lib.vd_hold_motion(self._h, mode))
        self.hold_motion = bool(on)

    def read_held(self, n, cap=None, out=None):
        """The held boxes H (label = age) of frames [0, n) of the last process() / hold()
        call (vd_read_held) as HostBoxes; cap defaults to the largest count. out: a
        HostBoxes / DeviceBoxes to fill instead (a device target is queued on the
        context stream, no host wait)."""
        return self._read_sized(lambda s: self._lib.vd_read_held(self._h, n, s), n, cap, out)

    def _read_sized(self, call, n, cap, out):
        """A reader's lists of frames [0, n): call(vd_boxes*) fills `out`, or a HostBoxes of
        `cap` boxes per frame; cap None: the counts are read first and cap is the largest."""
        if out is not None:
            s = out.struct()
            check(call(ctypes.byref(s)))
            return out
        if cap is None:
            cnt = _lib.HostBoxes(n, 1)
            s = cnt.struct()
            check(call(ctypes.byref(s)))
            cap = max(1, int(cnt.count.max()))
        boxes = _lib.HostBoxes(n, cap)
        s = boxes.struct()
        check(call(ctypes.byref(s)))
        return boxes

    # -- weak-detection rescue ------------------------------------------------------
    def rescue(self, rescue=0.0, plate_rescue=0.0, rescue_span=60):
        """vd_rescue: the low thresholds (0.0 / 0.0 = off) and the span. A change forgets the
        rescue and the hold history; it is refused while lead frames are pending and, unless
        rescue_tiles is on, in a tiling context."""
        lo, plo, span = _lib.check_rescue(rescue, plate_rescue, rescue_span)
        check(self._lib.vd_rescue(self._h, lo, plo, span))
        self.rescue_low, self.plate_rescue_low, self.rescue_span = lo, plo, span

    def set_rescue_tiles(self, on=True):
        """vd_rescue_tiles: whether rescue and tiling may be combined (1) or refuse each other (0, the
        default). Keeps every history; VdError while lead frames are pending, and for off while
        rescue and tiling are both on."""
        on = _lib.check_rescue_tiles(on)
        check(self._lib.vd_rescue_tiles(self._h, int(on)))
        self.rescue_tiles = on

    @staticmethod
    def _box_lists(boxes, none_if_empty=False):
        """A HostBoxes / DeviceBoxes as it is; a list with one int [k][4] array per frame as
        HostBoxes. none_if_empty: None or a list of no frames -> None."""
        if isinstance(boxes, (_lib.HostBoxes, DeviceBoxes)):
            return boxes
        if boxes is None and none_if_empty:
            return None
        lists = [np.asarray(b, np.int32).reshape(-1, 4) for b in boxes]
        if none_if_empty and not lists:
            return None
        det = _lib.HostBoxes(len(lists), max(1, max((len(b) for b in lists), default=1)))
        for i, b in enumerate(lists):
            det.count[i] = len(b)
            det.xyxy[i, :len(b)] = b
        return det

    def rescue_lists(self, strong, weak, h, w, out=None):
        """vd_rescue_lists: the rescue step alone, for callers with their own detectors. strong /
        weak: the strong and the weak detections of consecutive h x w frames -- HostBoxes /
        DeviceBoxes, or lists with one int [k][4] array per frame. Returns `out` (default: a
        HostBoxes with room for every box) holding E = D ++ R per frame, label = since (0: strong).
        Only the rescue history advances: hand E to hold()."""
        ds, dw = self._box_lists(strong), self._box_lists(weak)
        if ds.n != dw.n:
            raise ValueError(f"strong has {ds.n} frames, weak {dw.n}")
        if out is None:
            out = _lib.HostBoxes(ds.n, max(1, ds.cap + dw.cap))
        ss, sw, so = ds.struct(), dw.struct(), out.struct()
        check(self._lib.vd_rescue_lists(self._h, ctypes.byref(ss), ctypes.byref(sw), ds.n, int(h), int(w),
                                        ctypes.byref(so)))
        return out

    def read_rescue(self, net, n, which="rescued", cap=None, out=None):
        """The rescue step's lists of one net for frames [0, n) of the last process() /
        process_lead() call (vd_read_rescue) as HostBoxes: which="rescued" R (label = since, with
        the score), "weak" W (label and score as in the keep list). cap defaults to the largest
        count; out: a HostBoxes / DeviceBoxes to fill instead."""
        if which not in ("rescued", "weak"):
            raise ValueError(f"which {which!r}: expected 'rescued' or 'weak'")
        w = 0 if which == "rescued" else 1
        return self._read_sized(lambda s: self._lib.vd_read_rescue(self._h, net, n, w, s), n, cap, out)

    # -- look-ahead hold -----------------------------------------------------------
    def set_lead(self, lead=0, lead_motion=False):
        """vd_lead: blur a box up to `lead` frames (0 = off, at most 8) before its first
        detection; lead_motion stretches a led box backwards along the way the face came. A
        change while frames are pending is refused (lead_flush() or hold_reset() first)."""
        lead, lead_motion = _lib.check_lead(lead, lead_motion)
        mode = _lib.VD_HOLD_MOTION_LINEAR if lead_motion else _lib.VD_HOLD_MOTION_OFF
        check(self._lib.vd_lead(self._h, lead, mode))
        self.lead, self.lead_motion = lead, lead_motion

    @property
    def lead_delay(self):
        """Frames the output lags the input by: lead, one more with lead_motion."""
        return self.lead + (1 if self.lead_motion else 0)

    def lead_pending(self):
        """vd_lead_pending: frames pushed and not yet emitted."""
        k = ctypes.c_int(0)
        check(self._lib.vd_lead_pending(self._h, ctypes.byref(k)))
        return k.value

    def read_lead(self, n, which="lead", cap=None, out=None):
        """The lists of emitted frames [0, n) of the last process_lead() / lead_lists() call
        (vd_read_lead) as HostBoxes: which="lead" the led boxes A alone (label = -a: first seen
        a frames later), "all" the blur list B = D ++ H ++ A (labels 0, +a, -a). cap defaults
        to the largest count; out: a HostBoxes / DeviceBoxes to fill instead."""
        if which not in ("lead", "all"):
            raise ValueError(f"which {which!r}: expected 'lead' or 'all'")
        w = 0 if which == "lead" else 1
        if out is None and n == 0:
            return _lib.HostBoxes(0, 1)
        return self._read_sized(lambda s: self._lib.vd_read_lead(self._h, n, w, s), n, cap, out)

    def lead_lists(self, boxes, h, w, flush=False, out=None):
        """vd_lead_lists: the look-ahead step alone, for callers with their own detectors.
        boxes: the detections of consecutive h x w frames -- a HostBoxes / DeviceBoxes, a list
        with one int [k][4] array per frame, or None / [] (with flush=True: end the stream).
        Returns the blur lists B = D ++ H ++ A of the m frames this call emits (m = max(0,
        pending + n - delay), everything pending with flush) as HostBoxes of m rows, label 0 /
        +a / -a; with out= (room for pending + n rows) that target is filled and (out, m)
        returned."""
        det = self._box_lists(boxes, none_if_empty=True)
        n = det.n if det is not None else 0
        ds = det.struct() if det is not None else None
        m = ctypes.c_int(0)
        os_ = out.struct() if out is not None else None
        check(self._lib.vd_lead_lists(self._h, ctypes.byref(ds) if ds is not None else None, n, int(h), int(w),
                                      1 if flush else 0, ctypes.byref(os_) if os_ is not None else None,
                                      ctypes.byref(m)))
        if out is not None:
            return out, m.value
        return self.read_lead(m.value, "all")

    def process_lead(self, frames, out=None, faces=None, plates=None, flags=None, flush=False):
        """vd_process_lead: process() for a context with lead > 0. The frames are pushed --
        faces / plates are THEIR detections -- and the frames whose look-ahead is complete come
        back blurred with B = D ++ H ++ A: m = max(0, pending + n - delay) of them, everything
        pending with flush=True (the stream ends). frames may be None with flush=True.
        -> (out[:m], faces, plates); out defaults to a new array / tensor of pending + n
        frames. Under tiling a long batch is split into consecutive calls as by process(), and
        what they emit is concatenated."""
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        if frames is None:
            return self.lead_flush(out), faces, plates
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        room = self.lead_pending() + n
        if out is None:
            if where == _lib.VD_HOST:
                out = np.empty((room, h, w, 3), np.uint8)
            else:
                import torch
                out = torch.empty((room, h, w, 3), dtype=torch.uint8, device=frames.device)
        if len(out) and tuple(out.shape[1:]) != (h, w, 3):
            raise ValueError(f"out must be uint8 [m,{h},{w},3]")
        step = self._step(flags)
        if n > step and step < self.cfg.max_batch:
            pf, pp, m = [], [], 0
            for s0 in range(0, n, step):
                k = min(step, n - s0)
                o, f, q = self.process_lead(keep[s0:s0 + k], out[m:], _rows(faces, s0, k), _rows(plates, s0, k), flags,
                                            flush and s0 + k == n)
                m += len(o)
                pf.append(f)
                pp.append(q)
            if faces is None:
                faces = _host_concat(pf)
            if plates is None and flags & _lib.VD_PROC_PLATES:
                plates = _host_concat(pp)
            return out[:m], faces, plates
        fs = ps = None
        auto_f, auto_p = faces is None, plates is None
        if flags & _lib.VD_PROC_FACES:
            faces = self._boxes(faces, n)
            fs = faces.struct()
        if flags & _lib.VD_PROC_PLATES:
            plates = self._boxes(plates, n)
            ps = plates.struct()
        optr = out.data_ptr() if _is_torch(out) else ptr(out)
        m = ctypes.c_int(0)
        check(self._lib.vd_process_lead(self._h, p, n, h, w, pitch, where, flags,
                                        ctypes.byref(fs) if fs is not None else None,
                                        ctypes.byref(ps) if ps is not None else None,
                                        optr, len(out), 1 if flush else 0, ctypes.byref(m)))
        if flags & _lib.VD_PROC_FACES:
            faces = self._complete(faces, _lib.VD_NET_RETINAFACE, auto_f)
        if flags & _lib.VD_PROC_PLATES:
            plates = self._complete(plates, _lib.VD_NET_YOLOV8N, auto_p)
        self._lead_geom = (h, w, pitch, where, getattr(frames, "device", None))
        self._lead_nv12 = self._lead_yuv = None
        return out[:m.value], faces, plates

    def process_lead_nv12(self, frames, out=None, faces=None, plates=None, flags=None, flush=False, matrix="bt709",
                          range="limited", height=None):
        """vd_process_lead_nv12: process_lead() on NV12 frames (the layouts of process_nv12()). The
        surfaces are pushed -- faces / plates are THEIR detections, exactly process_lead()'s on
        nv12_to_rgb(frames) -- and the m surfaces whose look-ahead is complete come back with both
        planes blurred over B = D ++ H ++ A as mosaic_nv12() blurs them under the context's settings.
        The layout, matrix and range may change from call to call of one stream; h and w may not.
        frames may be None with flush=True. -> (out[:m], faces, plates); out defaults to new surfaces
        like the input, for pending + n frames."""
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        if frames is None:
            return self.lead_flush(out), faces, plates
        d, n, h, w, where, keep = _nv12_arg(frames, height, matrix, range)
        rows = int((frames.shape if _is_torch(frames) else np.shape(frames))[-2])
        dev = getattr(frames, "device", None) if _is_torch(frames) else None
        if out is None:
            out = self._nv12_new(self.lead_pending() + n, rows, w, where, dev)
        od = None
        if len(out):
            od, cap, oh, ow, owhere, okeep = _nv12_arg(out, height, writable=True)
            if (oh, ow, owhere) != (h, w, where):
                raise ValueError("out must hold NV12 frames of the input's h, w in the same memory (host / device)")
        m, faces, plates = self._lead_calls_420(self._lib.vd_process_lead_nv12, d, od, len(out), n, h, w, where, flags, faces,
                                                plates, flush)
        self._lead_nv12 = (h, w, rows, where, dev)
        self._lead_yuv = None
        del keep
        return out[:m], faces, plates

    def _lead_420(self, words, frames, out, faces, plates, flags, flush, layout, out_layout, depth, shift, matrix, range,
                  height):
        """What process_lead_yuv420() / process_lead_yuv420_16() share."""
        if flags is None:
            flags = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
        if frames is None:
            return self.lead_flush(out), faces, plates
        if words:
            d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height, matrix, range)
            fmt = (d.depth, d.shift)
            fn = self._lib.vd_process_lead_yuv420_16
        else:
            d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
            fmt = ()
            fn = self._lib.vd_process_lead_yuv420
        olay = out_layout or layout
        src = frames.buffer if isinstance(frames, (Yuv420, Yuv420_16)) else frames
        dev = src.device if _is_torch(src) else None
        if out is None:
            out = self._yuv420_new(self.lead_pending() + n, h, w, dev, words)
            oheight = None
        else:
            oheight = height
        od, cap = None, (out.n if isinstance(out, (Yuv420, Yuv420_16)) else len(out))
        if cap:
            if words:
                od, cap, oh, ow, owhere, okeep = _yuv420_16_arg(out, olay, *fmt, oheight, writable=True)
            else:
                od, cap, oh, ow, owhere, okeep = _yuv420_arg(out, olay, oheight, writable=True)
            if (oh, ow, owhere) != (h, w, where):
                raise ValueError("out must hold 4:2:0 frames of the input's h, w in the same memory (host / device)")
        m, faces, plates = self._lead_calls_420(fn, d, od, cap, n, h, w, where, flags, faces, plates, flush)
        self._lead_yuv = (words, h, w, dev, olay, fmt)
        self._lead_nv12 = None
        del keep
        return (out if isinstance(out, (Yuv420, Yuv420_16)) else out[:m]), faces, plates

    def process_lead_yuv420(self, frames, out=None, faces=None, plates=None, flags=None, flush=False, layout="i420",
                            out_layout=None, matrix="bt709", range="limited", height=None):
        """vd_process_lead_yuv420: process_lead_nv12() on 8-bit 4:2:0 frames in any layout (the argument
        forms of process_yuv420()). Lists and every emitted sample are exactly process_lead_nv12()'s on
        the NV12 frames with the same samples; in and out layouts are independent and either may change
        from call to call (h and w may not); one stream may be pushed by this call and
        process_lead_nv12() in turn. out defaults to new packed surfaces for pending + n frames in
        `out_layout or layout`, in the memory the input lives in. frames may be None with flush=True.
        -> (out[:m], faces, plates); a Yuv420 out comes back whole, its first m surfaces written
        (m = the drop in lead_pending() + n)."""
        return self._lead_420(False, frames, out, faces, plates, flags, flush, layout, out_layout, None, None, matrix, range,
                              height)

    def process_lead_yuv420_16(self, frames, out=None, faces=None, plates=None, flags=None, flush=False, layout="i420",
                               out_layout=None, matrix="bt709", range="limited", height=None, depth=10, shift=None):
        """vd_process_lead_yuv420_16: process_lead_yuv420() on 10- or 12-bit 4:2:0 frames (the argument
        forms of process_yuv420_16()). Lists are exactly process_lead_yuv420()'s on the frames' 8-bit
        picture; the blur acts on the 16-bit samples and every word no box owns comes back as it was.
        out keeps the input's depth and shift, which must not change while surfaces are pending.
        -> (out[:m], faces, plates)."""
        return self._lead_420(True, frames, out, faces, plates, flags, flush, layout, out_layout, depth, shift, matrix, range,
                              height)

    @staticmethod
    def _yuv420_new(n, h, w, dev, words):
        """n new packed 4:2:0 surfaces [n, 3h/2, w], 8-bit or 16-bit words, on the host or on `dev`."""
        if dev is None:
            return np.empty((n, h // 2 * 3, w), np.uint16 if words else np.uint8)
        import torch
        return torch.empty((n, h // 2 * 3, w), dtype=torch.int16 if words else torch.uint8, device=dev)

    def _lead_flush_yuv(self, out, pend):
        words, h, w, dev, olay, fmt = self._lead_yuv
        if out is None:
            out = self._yuv420_new(pend, h, w, dev, words)
        whole = isinstance(out, (Yuv420, Yuv420_16))
        cap = out.n if whole else len(out)
        if pend == 0 or cap == 0:
            if pend:
                raise _lib.VdCapacityError(_lib.VD_ERR_CAPACITY, f"{pend} frames to emit, out holds 0")
            return out if whole else out[:0]
        if words:
            od, cap, oh, ow, owhere, okeep = _yuv420_16_arg(out, olay, *fmt, h, writable=True)
            fn = self._lib.vd_process_lead_yuv420_16
        else:
            od, cap, oh, ow, owhere, okeep = _yuv420_arg(out, olay, h, writable=True)
            fn = self._lib.vd_process_lead_yuv420
        m = ctypes.c_int(0)
        check(fn(self._h, None, ctypes.byref(od), 0, h, w, owhere, _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC, None, None, cap,
                 1, ctypes.byref(m)))
        del okeep
        return out if whole else out[:m.value]

    @staticmethod
    def _nv12_new(n, rows, w, where, dev):
        """n new packed surfaces of `rows` rows (3/2 of the, possibly padded, luma height) by w."""
        if where == _lib.VD_HOST and dev is None:
            return np.empty((n, rows, w), np.uint8)
        import torch
        return torch.empty((n, rows, w), dtype=torch.uint8, device=dev)

    def _lead_flush_nv12(self, out, pend):
        h, w, rows, where, dev = self._lead_nv12
        if out is None:
            out = self._nv12_new(pend, rows, w, where, dev)
        if pend == 0 or len(out) == 0:
            if pend:
                raise _lib.VdCapacityError(_lib.VD_ERR_CAPACITY, f"{pend} frames to emit, out holds 0")
            return out[:0]
        od, cap, oh, ow, owhere, okeep = _nv12_arg(out, h, writable=True)
        m = ctypes.c_int(0)
        check(self._lib.vd_process_lead_nv12(self._h, None, ctypes.byref(od), 0, h, w, owhere,
                                             _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC, None, None, cap, 1,
                                             ctypes.byref(m)))
        del okeep
        return out[:m.value]

    def lead_flush(self, out=None):
        """End the stream: the pending frames of process_lead() leave, blurred with what is
        known (vd_process_lead with n == 0 and flush). -> out[:m]; out defaults to a new array
        / tensor like the frames pushed last. Pending frames of process_lead_nv12() leave as NV12
        surfaces (vd_process_lead_nv12), host or device as they were pushed, with their luma height;
        those of process_lead_yuv420() / process_lead_yuv420_16() as packed surfaces in the family, the
        (output) layout, depth and shift of the last push."""
        pend = self.lead_pending()
        if getattr(self, "_lead_yuv", None) is not None:
            return self._lead_flush_yuv(out, pend)
        if getattr(self, "_lead_nv12", None) is not None:
            return self._lead_flush_nv12(out, pend)
        geom = getattr(self, "_lead_geom", None)
        if pend == 0 or geom is None:
            if out is not None:
                return out[:0]
            return np.empty((0, 0, 0, 3), np.uint8)
        h, w, pitch, where, dev = geom
        if out is None:
            if where == _lib.VD_HOST:
                out = np.empty((pend, h, w, 3), np.uint8)
            else:
                import torch
                out = torch.empty((pend, h, w, 3), dtype=torch.uint8, device=dev)
        where = (_lib.VD_DEVICE if out.is_cuda else _lib.VD_HOST) if _is_torch(out) else _lib.VD_HOST
        optr = out.data_ptr() if _is_torch(out) else ptr(out)
        m = ctypes.c_int(0)
        check(self._lib.vd_process_lead(self._h, None, 0, h, w, pitch, where,
                                        _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC, None, None, optr, len(out), 1,
                                        ctypes.byref(m)))
        return out[:m.value]

    # -- mask shaping -----------------------------------------------------------
    def set_mask(self, mask="rect", mask_grow=0):
        """vd_mask: the shape ("rect" | "ellipse") and the margin (percent, 0..200) of what the
        next blurring call hides; ("rect", 0) is the detector's rectangle."""
        mask, mask_grow = _lib.check_mask(mask, mask_grow)
        check(self._lib.vd_mask(self._h, _lib.MASK_SHAPES[mask], mask_grow))
        self.mask, self.mask_grow = mask, mask_grow

    def mask_boxes(self, boxes, out=None):
        """vd_mask_boxes: the boxes as the context's blurring calls grow them (mask_grow; the
        shape plays no part), by the kernel of the blur path. boxes: a HostBoxes / DeviceBoxes,
        or a list with one int [k][4] array per frame. Returns `out` (default: host lists for
        host boxes, a DeviceBoxes for device boxes, of the same cap): counts as given, xyxy
        grown, nothing else written."""
        src = self._box_lists(boxes)
        if out is None:
            out = (DeviceBoxes(src.n, src.cap, src.xyxy.device) if isinstance(src, DeviceBoxes)
                   else _lib.HostBoxes(src.n, src.cap))
        ss, os_ = src.struct(), out.struct()
        check(self._lib.vd_mask_boxes(self._h, ctypes.byref(ss), src.n, ctypes.byref(os_)))
        return out

    # -- box-scaled strength -------------------------------------------------------
    def set_cells(self, cells=0):
        """vd_cells: at most `cells` (2..64) cells across every box from the next blurring call
        on; 0 is off (the constant mosaic_level / blur_ksize)."""
        cells = _lib.check_cells(cells)
        check(self._lib.vd_cells(self._h, cells))
        self.cells = cells

    # -- tiled detection -----------------------------------------------------------
    def set_tiles(self, tiles=(1, 1), tile_overlap=20):
        """vd_tiles: the tiling (rows, cols) and the overlap percentage (0..50) of the face
        detection from the next call on; (1, 1) is off. A change forgets the hold history (and,
        with rescue_tiles in a rescue context, the rescue history)."""
        tiles, tile_overlap = _lib.check_tiles(tiles, tile_overlap)
        check(self._lib.vd_tiles(self._h, tiles[0], tiles[1], tile_overlap))
        self.tiles, self.tile_overlap = tiles, tile_overlap

    def set_tile_nets(self, tile_nets="faces"):
        """vd_tiles_nets: which nets the tiling applies to from the next call on: "faces" (the
        default), "plates" or "both". A change while tiling is on forgets the hold history."""
        tile_nets = _lib.check_tile_nets(tile_nets)
        check(self._lib.vd_tiles_nets(self._h, _lib.TILE_NETS[tile_nets]))
        self.tile_nets = tile_nets

    def set_tile_surfaces(self, on=True):
        """vd_tiles_surfaces: whether the 4:2:0 surface calls run the tiled nets (1) or refuse a call
        that would (0, the default). Keeps the hold history; VdError while lead frames are pending."""
        check(self._lib.vd_tiles_surfaces(self._h, int(on)))
        self.tile_surfaces = bool(on)

    def tile_rects(self, h, w):
        """The net inputs' rectangles (x, y, w, h) of an h x w frame under the context's tiling
        (vd_tile_rects): int32 [T][4], row 0 the whole frame."""
        return _lib.tile_rects(h, w, self.tiles, self.tile_overlap)

    def tiles_merge(self, lists, h, w, out=None):
        """vd_tiles_merge: the cross-tile merge alone. lists: a HostBoxes / DeviceBoxes of n * T
        rows (frame f's input t at row f * T + t; xyxy_f, score, label read), boxes relative to
        their rectangle of an h x w frame. Returns `out` (default: HostBoxes with the complete
        merged lists): the mapped boxes in merged order, label = t * A + the input's label."""
        T = 1 + self.tiles[0] * self.tiles[1]
        n = lists.n // T
        ls = lists.struct()
        if out is not None:
            s = out.struct()
            check(self._lib.vd_tiles_merge(self._h, ctypes.byref(ls), n, int(h), int(w), ctypes.byref(s)))
            return out
        check(self._lib.vd_tiles_merge(self._h, ctypes.byref(ls), n, int(h), int(w), None))
        return self.read_boxes(_lib.VD_NET_RETINAFACE, n)

    def tiles_merge_plates(self, lists, h, w, out=None):
        """vd_tiles_merge_plates: the plate merge alone, the counterpart of tiles_merge(): the same
        layout of `lists`, label read as the class. Returns `out` (default: HostBoxes with the
        complete merged lists): the mapped boxes in merged order, label = the class."""
        T = 1 + self.tiles[0] * self.tiles[1]
        n = lists.n // T
        ls = lists.struct()
        if out is not None:
            s = out.struct()
            check(self._lib.vd_tiles_merge_plates(self._h, ctypes.byref(ls), n, int(h), int(w), ctypes.byref(s)))
            return out
        check(self._lib.vd_tiles_merge_plates(self._h, ctypes.byref(ls), n, int(h), int(w), None))
        return self.read_boxes(_lib.VD_NET_YOLOV8N, n)

    def tiles_merge_low(self, lists, h, w, thr, plates=False, cap=None, strong=None):
        """vdt_tiles_merge_low: the merge in its rescue form alone. lists: as tiles_merge() /
        tiles_merge_plates() take them, read as the lists at the low threshold; thr: the net's
        threshold (faces score >= thr, plates score > thr are strong). Returns (strong, whole): the
        caller-shaped strong list exactly as the merge writes it (a HostBoxes to fill, or a new one
        of cap boxes per frame, default: room for every box; count complete) and the whole merged
        rows with the whole merged count."""
        T = 1 + self.tiles[0] * self.tiles[1]
        n = lists.n // T
        full = max(1, T * lists.cap)
        if strong is None:
            strong = _lib.HostBoxes(n, full if cap is None else cap)
        whole = _lib.HostBoxes(n, full)
        ls, ss, ws = lists.struct(), strong.struct(), whole.struct()
        check(self._lib.vdt_tiles_merge_low(self._h, ctypes.byref(ls), n, int(h), int(w), 1 if plates else 0, float(thr),
                                            ctypes.byref(ss), ctypes.byref(ws)))
        return strong, whole

    def _letterbox_tiles_420(self, fn, d, n, h, w, where, cpad):
        T = 1 + self.tiles[0] * self.tiles[1]
        out = np.zeros((n * T, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(fn(self._h, ctypes.byref(d), n, h, w, where, ptr(out), cpad))
        return out

    def letterbox_tiles_nv12(self, frames, cpad=4, matrix="bt709", range="limited", height=None):
        """vdt_letterbox_tiles_nv12: letterbox_tiles() of NV12 frames by the tile letterbox kernel with the
        NV12 pixel source (what the *_nv12 entries run); tile_surfaces is not read."""
        d, n, h, w, where, keep = _nv12_arg(frames, height, matrix, range)
        return self._letterbox_tiles_420(self._lib.vdt_letterbox_tiles_nv12, d, n, h, w, where, cpad)

    def letterbox_tiles_yuv420(self, frames, cpad=4, layout="i420", matrix="bt709", range="limited", height=None):
        """vdt_letterbox_tiles_yuv420: letterbox_tiles() of 4:2:0 frames in any layout."""
        d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
        return self._letterbox_tiles_420(self._lib.vdt_letterbox_tiles_yuv420, d, n, h, w, where, cpad)

    def letterbox_tiles_yuv420_16(self, frames, cpad=4, layout="i420", depth=10, shift=None, matrix="bt709",
                                  range="limited", height=None):
        """vdt_letterbox_tiles_yuv420_16: letterbox_tiles() of 10- / 12-bit 4:2:0 frames."""
        d, n, h, w, where, keep = _yuv420_16_arg(frames, layout, depth, shift, height, matrix, range)
        return self._letterbox_tiles_420(self._lib.vdt_letterbox_tiles_yuv420_16, d, n, h, w, where, cpad)

    def letterbox_tiles(self, frames, cpad=4):
        """vdt_letterbox_tiles: letterbox() for the n * T canvases of a tiling context, canvas
        f * T + t; a torch view with padded rows is read at its own row pitch."""
        p, n, h, w, pitch, where, keep = _frames_arg(frames, pitched=True)
        T = 1 + self.tiles[0] * self.tiles[1]
        out = np.zeros((n * T, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(self._lib.vdt_letterbox_tiles(self._h, p, n, h, w, pitch, where, ptr(out), cpad))
        return out

    # -- frame I/O ------------------------------------------------------------
    def jpeg_decode(self, jpegs, out=None):
        """Baseline JPEG frames (a list of bytes, all one size and layout) -> RGB
        uint8 [n,h,w,3], bit-identical to libjpeg-turbo's default decode (what
        cv2.imread + BGR->RGB gives the reference, combine_detect.py:167-172).
        `out`: a torch uint8 device tensor (decoded in place on the GPU, queued on
        the context stream -- ready to pass to process()) or None (numpy result)."""
        jpegs = [bytes(j) for j in jpegs]
        n = len(jpegs)
        if n == 0:
            raise ValueError("no frames")
        h, w, _ = jpeg_info(jpegs[0])
        # the bytes objects' own buffers (immutable; the library only reads them): no copy
        bufs = [ctypes.c_char_p(j) for j in jpegs]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
        sizes = (ctypes.c_size_t * n)(*[len(j) for j in jpegs])
        if out is None:
            out = np.empty((n, h, w, 3), np.uint8)
        if _is_torch(out):
            if tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous():
                raise ValueError(f"out must be contiguous uint8 [{n},{h},{w},3]")
            where, optr = (_lib.VD_DEVICE if out.is_cuda else _lib.VD_HOST), out.data_ptr()
        else:
            if out.shape != (n, h, w, 3) or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]:
                raise ValueError(f"out must be C-contiguous uint8 [{n},{h},{w},3]")
            where, optr = _lib.VD_HOST, ptr(out)
        check(self._lib.vd_jpeg_decode(self._h, ptrs, sizes, n, optr, h, w, w * 3, where))
        return out

    def jdec_passes(self):
        """Synchronisation passes of the last jpeg_decode's device entropy stage (pass 0
        included; 0 when the host entropy stage ran) -- test / bench hook."""
        p = ctypes.c_int(0)
        check(self._lib.vdt_jdec_stats(self._h, ctypes.byref(p)))
        return p.value

    def jpeg_encode(self, frames, quality=95, subsampling=2, copy=True):
        """RGB uint8 frames [n,h,w,3] (numpy, or a torch tensor on the GPU: encoded
        from device memory, no D2H of pixels) -> list of JFIF bytes, bit-identical to
        libjpeg-turbo's compressor (Pillow ``Image.save(..., quality=quality,
        subsampling=subsampling)``; cv2.imwrite's defaults are quality 95, 4:2:0 --
        the reference's frame write, combine_detect.py:174-180).
        copy=False: read-only memoryviews into one buffer of this call (no per-frame
        copy into bytes objects; the buffer lives as long as any view does).
        """
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        sizes = (ctypes.c_size_t * n)()
        # typical frames need < 3 B/pixel; on VD_ERR_CAPACITY the device coder reports
        # each frame's bound in sizes[] (the host coder 0: then the bound of any
        # baseline block, 63 AC codes of 26 bits + DC, every byte stuffed)
        caps = [h * w * 3 + 65536]
        while len(caps) < 3:
            cap = caps[-1]
            if copy:   # one staging buffer per context, reused (fresh pages would fault in on every call)
                out = getattr(self, "_jenc_buf", None)
                if out is None or out.size < n * cap:
                    out = self._jenc_buf = np.empty(n * cap, np.uint8)
            else:      # this call's own buffer: the views stay valid (first touch on the copy threads)
                out = np.empty(n * cap, np.uint8)
            rc = self._lib.vd_jpeg_encode(self._h, p, n, h, w, pitch, where, int(quality), int(subsampling),
                                          ptr(out), cap, sizes)
            if rc != _lib.VD_ERR_CAPACITY:
                break
            need = max(sizes[i] for i in range(n))
            caps.append(need + 64 if need > cap else h * w * 20 + 65536)
        check(rc)
        del keep
        if not copy:
            mv = memoryview(out).toreadonly()
            return [mv[i * cap:i * cap + sizes[i]] for i in range(n)]
        return [out[i * cap:i * cap + sizes[i]].tobytes() for i in range(n)]

    # -- instrumentation ------------------------------------------------------
    def timing(self, on=True):
        check(self._lib.vd_timing_enable(self._h, 1 if on else 0))

    def timing_reset(self):
        check(self._lib.vd_timing_reset(self._h))

    def timing_read(self, fam):
        ms, n, work = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        check(self._lib.vd_timing_read(self._h, fam, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(work)))
        return ms.value, n.value, work.value

    # -- test hooks --------------------------------------------------------------
    def letterbox(self, frames, cpad=4):
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        out = np.zeros((n, self.cfg.input_h, self.cfg.input_w, cpad), np.float32)
        check(self._lib.vdt_letterbox(self._h, p, n, h, w, pitch, where, ptr(out), cpad))
        return out

    def forward_heads(self, frames):
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        A = sum((self.cfg.input_h // s) * (self.cfg.input_w // s) * 2 for s in (8, 16, 32))
        loc = np.zeros((n, A, 4), np.float32)
        conf = np.zeros((n, A, 2), np.float32)
        landm = np.zeros((n, A, 10), np.float32)
        check(self._lib.vdt_forward_heads(self._h, p, n, h, w, pitch, where, ptr(loc), ptr(conf), ptr(landm)))
        return loc, conf, landm

    def face_band_stats(self):
        """Letterbox bands of the last face forward (vdt_face_band_stats): int32 [4][5], per band op
        (stem + pool, layer1.0-2) lo, hi, tile rows, frames whose band tiles were left alone, frames
        whose band tiles ran; zeros for a forward that ran without bands."""
        out = np.zeros((4, 5), np.int32)
        check(self._lib.vdt_face_band_stats(self._h, ptr(out)))
        return out

    def postprocess(self, loc, conf, img_hw, cap=None):
        loc = np.ascontiguousarray(loc, np.float32)
        conf = np.ascontiguousarray(conf, np.float32)
        n = loc.shape[0]
        hw = np.ascontiguousarray(np.broadcast_to(np.asarray(img_hw, np.int32), (n, 2)))
        boxes = _lib.HostBoxes(n, cap or self.cfg.max_boxes)
        s = boxes.struct()
        check(self._lib.vdt_postprocess(self._h, ptr(loc), ptr(conf), n, ptr(hw), ctypes.byref(s)))
        return self._complete(boxes, _lib.VD_NET_RETINAFACE, cap is None)

    def plate_raw(self, frames):
        """Raw YOLO head outputs [n][64+nc][A] (DFL logits | class logits), f32."""
        p, n, h, w, pitch, where, keep = _frames_arg(frames)
        A = ctypes.c_int()
        check(self._lib.vdt_plate_raw(self._h, p, n, h, w, pitch, where, None, ctypes.byref(A)))
        out = np.zeros((n, 64 + self.cfg.plate_nc, A.value), np.float32)
        check(self._lib.vdt_plate_raw(self._h, p, n, h, w, pitch, where, ptr(out), ctypes.byref(A)))
        return out

    def plate_raw_tiles(self, frames):
        """vdt_plate_raw_tiles: plate_raw() of the n * R * C tile inputs of a tiling context, input
        f * R * C + (t - 1); a torch view with padded rows is read at its own row pitch."""
        p, n, h, w, pitch, where, keep = _frames_arg(frames, pitched=True)
        ni = n * self.tiles[0] * self.tiles[1]
        A = ctypes.c_int()
        check(self._lib.vdt_plate_raw_tiles(self._h, p, n, h, w, pitch, where, None, ctypes.byref(A)))
        out = np.zeros((ni, 64 + self.cfg.plate_nc, A.value), np.float32)
        check(self._lib.vdt_plate_raw_tiles(self._h, p, n, h, w, pitch, where, ptr(out), ctypes.byref(A)))
        return out

    def plate_raw_tiles_yuv420(self, frames, layout="i420", matrix="bt709", range="limited", height=None):
        """vdt_plate_raw_tiles_yuv420: plate_raw_tiles() of 4:2:0 frames in any layout, by the tile-only
        letterbox kernel with the surfaces' pixel source; tile_surfaces is not read."""
        d, n, h, w, where, keep = _yuv420_arg(frames, layout, height, matrix, range)
        ni = n * self.tiles[0] * self.tiles[1]
        A = ctypes.c_int(0)
        check(self._lib.vdt_plate_raw_tiles_yuv420(self._h, ctypes.byref(d), n, h, w, where, None, ctypes.byref(A)))
        out = np.zeros((ni, 64 + self.cfg.plate_nc, A.value), np.float32)
        check(self._lib.vdt_plate_raw_tiles_yuv420(self._h, ctypes.byref(d), n, h, w, where, ptr(out), ctypes.byref(A)))
        del keep
        return out

    def plate_postprocess(self, raw, img_hw, cap=None):
        """vdt_plate_postprocess: the plate post kernels on raw heads [n][64+nc][A] as plate_raw()
        returns them, for frames of img_hw whose canvas the last plate forward was run for."""
        raw = np.ascontiguousarray(raw, np.float32)
        n = raw.shape[0]
        boxes = _lib.HostBoxes(n, cap or self.cfg.max_boxes)
        s = boxes.struct()
        check(self._lib.vdt_plate_postprocess(self._h, ptr(raw), n, int(img_hw[0]), int(img_hw[1]), ctypes.byref(s)))
        return self._complete(boxes, _lib.VD_NET_YOLOV8N, cap is None)

    def bottleneck(self, x, w1, bn1, w2, bn2, w3, bn3, wd=None, bnd=None, fused=True):
        """One ResNet layer1 bottleneck (bf16 or fp32 context): x f32 NHWC [n,h,w,cin] -> f32
        NHWC [n,h,w,256]; bnK = concat(scale, shift). fused: the one-kernel block
        (block.hip / block32.hip), else the conv-by-conv chain."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        x = f(x)
        n, h, wd_, cin = x.shape
        y = np.zeros((n, h, wd_, 256), np.float32)
        args = [f(a) for a in (w1, bn1, w2, bn2, w3, bn3, wd, bnd)]
        check(self._lib.vdt_bottleneck(self._h, ptr(x), n, h, wd_, cin, *[ptr(a) for a in args], int(bool(fused)),
                                       ptr(y)))
        return y

    def conv2d(self, x, w, stride=1, pad=0, scale=None, shift=None, act=0, slope=0.0, res=None, res_mode=0):
        """x: f32 NHWC [n,h,w,cin]; w: f32 [cout,cin,kh,kw] -> f32 NHWC."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        n, h, wd, cin = x.shape
        cout, _, kh, kw = w.shape
        scale = np.ascontiguousarray(np.ones(cout, np.float32) if scale is None else scale, np.float32)
        shift = np.ascontiguousarray(np.zeros(cout, np.float32) if shift is None else shift, np.float32)
        oh, ow = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
        y = np.zeros((n, oh, ow, cout), np.float32)
        r = None if res is None else np.ascontiguousarray(res, np.float32)
        o1, o2 = ctypes.c_int(), ctypes.c_int()
        check(self._lib.vdt_conv2d(self._h, ptr(x), n, h, wd, cin, ptr(w), cout, kh, kw, stride, pad, ptr(scale),
                                   ptr(shift), act, float(slope), ptr(r), res_mode, ptr(y), ctypes.byref(o1),
                                   ctypes.byref(o2)))
        return y

    def run_op(self, kind, x, y, *, xcoff=0, ycoff=0, y_is_x=False, out16=True, f0=0, n=None,
               w=None, scale=None, shift=None, stride=1, pad=0, act=0, slope=0.0, grp_co=0, grp_ci=0,
               res=None, res_coff=0, res_mode=0, res_up=False, r_is_y=False,
               x2=None, w2=None, scale2=None, shift2=None, stride2=1,
               ch=0, k=0, s=0, p=0, yslots=None):
        """vdt_run_op: one plan op ("conv" | "maxpool" | "upsample" | "dwconv") through the production
        executor on whole NHWC buffers. x [frames,xh,xw,ldx] and y [frames,yh,yw,ldy] are f32 images of
        the buffers (y: the prior contents; with y_is_x pass y=None, the output lies in x's buffer);
        res [frames,rh,rw,res_ld] / x2 [frames,xh2,xw2,ldx2] likewise. Conv weights w [cout,cin,kh,kw]
        (dwconv: [c,3,3] or [c,1,3,3]). Returns a dict: y (the y buffer after the op), family (the
        dispatch record), and in the fp16-pair plan xslots / yslots [frames] (else None)."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        x = f(x)
        o = _lib.vdt_op()
        o.kind = {"conv": _lib.VDT_OP_CONV, "maxpool": _lib.VDT_OP_MAXPOOL, "upsample": _lib.VDT_OP_UPSAMPLE,
                  "dwconv": _lib.VDT_OP_DWCONV}[kind]
        frames = x.shape[0]
        o.frames, o.f0, o.n = frames, int(f0), int(frames - f0 if n is None else n)
        o.x, (o.xh, o.xw, o.ldx), o.xcoff = ptr(x), x.shape[1:], int(xcoff)
        yb = np.zeros_like(x) if y_is_x else f(y).copy()
        assert yb.shape[0] == frames
        o.y, (o.yh, o.yw, o.ldy), o.ycoff = ptr(yb), yb.shape[1:], int(ycoff)
        o.y_is_x, o.r_is_y, o.out16 = int(bool(y_is_x)), int(bool(r_is_y)), int(bool(out16))
        keep = [x, yb]
        if res is not None:
            res = f(res)
            assert res.shape[0] == frames
            o.res, (o.rh, o.rw, o.res_ld) = ptr(res), res.shape[1:]
            keep.append(res)
        o.res_coff, o.res_mode, o.res_up = int(res_coff), int(res_mode), int(bool(res_up))
        if kind in ("conv", "dwconv"):
            w = f(w)
            if kind == "dwconv":
                w = np.ascontiguousarray(w.reshape(w.shape[0], 3, 3))
                o.cin = o.cout = w.shape[0]
                o.kh = o.kw = 3
                o.pad = 1
            else:
                o.cout, o.cin, o.kh, o.kw = w.shape
                o.pad = int(pad)
            cout = w.shape[0]
            scale = f(np.ones(cout) if scale is None else scale)
            shift = f(np.zeros(cout) if shift is None else shift)
            assert scale.shape == (cout,) and shift.shape == (cout,)
            o.w, o.scale, o.shift = ptr(w), ptr(scale), ptr(shift)
            o.stride, o.act, o.slope = int(stride), int(act), float(slope)
            o.grp_co, o.grp_ci = int(grp_co), int(grp_ci)
            keep += [w, scale, shift]
            if x2 is not None:
                x2, w2 = f(x2), f(w2)
                assert x2.shape[0] == frames and w2.shape[0] == cout and w2.shape[2:] == (1, 1)
                scale2 = f(np.ones(cout) if scale2 is None else scale2)
                shift2 = f(np.zeros(cout) if shift2 is None else shift2)
                o.x2, (o.xh2, o.xw2, o.ldx2) = ptr(x2), x2.shape[1:]
                o.cin2, o.stride2 = w2.shape[1], int(stride2)
                o.w2, o.scale2, o.shift2 = ptr(w2), ptr(scale2), ptr(shift2)
                keep += [x2, w2, scale2, shift2]
        o.ch, o.k, o.s, o.p = int(ch), int(k), int(s), int(p)
        xs = np.zeros(frames, np.float32)
        ys = np.zeros(frames, np.float32) if yslots is None else f(yslots).copy()
        assert ys.shape == (frames,)
        o.xslots, o.yslots = ptr(xs), ptr(ys)
        check(self._lib.vdt_run_op(self._h, ctypes.byref(o)))
        del keep
        ranged = bool(o.ranged)
        return dict(y=yb, family=o.family.decode(), xslots=xs if ranged else None, yslots=ys if ranged else None)
