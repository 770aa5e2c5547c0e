"""vdmi — MI355X-native detect-and-blur hot path of Video-desensitization.

Host-side mirror of the reference's per-frame interfaces over libvdmi.so
(include/vdmi.h):

* ``Retinaface``                       detect_face/face.py:14-150
* ``YOLO`` / ``PlateDetector``         ultralytics call at combine_detect.py:217,872
* ``mosaic_rectangle_region_single``   combine_detect.py:138-161
* ``gaussian_blur_region_single``      its Gaussian-blur counterpart (blur="gaussian")
* ``batch_process_images``             combine_detect.py:183-277 (hot-loop body on GPU)
* ``Context``                          the C-ABI context (device frames, timing hooks)
"""
from ._lib import VdCapacityError, VdError, load  # noqa: F401
from .context import Context, DeviceBoxes, Yuv420, Yuv420_16, jpeg_info, nv12_to_rgb, yuv420_to_rgb, yuv420_16_to_rgb  # noqa: F401
from .face import Retinaface  # noqa: F401
from .mosaic import (blur_frames, gaussian_blur_region_single, mosaic_frames,  # noqa: F401
                     mosaic_rectangle_region_single, smooth_frames)
from .plate import YOLO, PlateDetector  # noqa: F401

__all__ = ["Context", "DeviceBoxes", "Retinaface", "YOLO", "PlateDetector", "mosaic_rectangle_region_single",
           "mosaic_frames", "gaussian_blur_region_single", "blur_frames", "smooth_frames", "VdError", "VdCapacityError", "load", "jpeg_info", "nv12_to_rgb", "Yuv420", "yuv420_to_rgb", "Yuv420_16", "yuv420_16_to_rgb"]
