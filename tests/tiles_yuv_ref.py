"""numpy reference of the rectangle form of a 4:2:0 pixel source (include/vdmi.h at vd_tiles_surfaces),
written from the definition, not from the kernel. A rectangle of a 4:2:0 frame at origin (y0, x0) is
read as
  the luma plane from (y0, x0),
  the chroma planes from sample (y0 >> 1, x0 >> 1) of the FRAME,
  the origin's parities (py, px) = (y0 & 1, x0 & 1):
local pixel (yy, x) takes luma (yy, x), chroma row (py + yy) >> 1 and chroma sample (px + x) >> 1, all
counted from those three origins. Planes are plain arrays (Y [h, w], U and V [h/2, w/2], 8-bit samples,
or the 8-bit picture of wider ones), so the form is the same for every layout."""
import numpy as np

import nv12_ref as nr


def rect_source(Y, U, V, x0, y0):
    """(luma view, U view, V view, py, px): what a rectangle source at origin (y0, x0) holds."""
    return Y[y0:, x0:], U[y0 >> 1:, x0 >> 1:], V[y0 >> 1:, x0 >> 1:], y0 & 1, x0 & 1


def staged_chroma_samples(px, iw):
    """Chroma samples the iw pixels of one row of a rectangle need, from the one of its first pixel."""
    return (px + iw + 1) >> 1


def rect_to_rgb(Y, U, V, x0, y0, tw, th, matrix="bt709", rng="limited"):
    """uint8 [th, tw, 3]: the conversion of the tw x th rectangle at (y0, x0) through the rectangle form.
    Every index is checked against the frame, as the kernel's loads have to stay inside it."""
    Yr, Ur, Vr, py, px = rect_source(np.asarray(Y), np.asarray(U), np.asarray(V), x0, y0)
    yy, xx = np.arange(th)[:, None], np.arange(tw)[None, :]
    cy, cx = (py + yy) >> 1, (px + xx) >> 1
    assert th <= Yr.shape[0] and tw <= Yr.shape[1], "the rectangle lies inside the frame"
    assert int(cy.max()) < Ur.shape[0] and int(cx.max()) < Ur.shape[1], "its chroma samples too"
    assert int(cx.max()) == staged_chroma_samples(px, tw) - 1, "a staged row holds exactly the samples the row reads"
    return nr.convert(Yr[yy, xx], Ur[cy, cx], Vr[cy, cx], matrix, rng)
