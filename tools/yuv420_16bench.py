"""10-bit 4:2:0 against NV12 and I420 at 1080p: the output pass (timing family 1) and the face letterbox
(family 2) of 64 device surfaces in 4-frame steps, all in one session.

    python tools/yuv420_16bench.py --parent-lib PATH/libvdmi.so [--repeats 5] [--passes 3]
                                   [--json profiles/yuv420_16_1080p.json]

A child process per measurement (a fresh context, a fresh library), the parent commit's build and this
build alternating, `--repeats` of each; every figure is reported as median (min .. max) over the runs.
    parent   the PARENT commit's build (through VDMI_LIB; the *_yuv420_16 entries are not bound):
               nv12   NV12 surfaces through the *_nv12 entries
               i420   I420 in and out through the *_yuv420 entries
    this     this build: nv12 and i420 as above, and
               p010   P010 in and out (depth 10, shift 6, interleaved) through the *_yuv420_16 entries
               p10    yuv420p10le in and out (depth 10, shift 0, planar)
Per case, over the face lists detected on synth's RGB frames of the same size (the dense box set of
tools/cellsbench.py, some 31 boxes a frame): ms per 4-frame step of
    mosaic      family 1 of mosaic_* (pixelation, level 8): one launch
    smooth      family 1 of smooth_* (level 8, cells 16): the copy and the box pass
    letterbox   family 2 of process_* with VD_PROC_FACES: the face letterbox
each the mean over `--passes` passes over the 16 steps after one warm-up pass, events around every launch,
with the bytes the library itself books for the launches (a 16-bit surface: twice an 8-bit one's).
Two expectations are reported as holds / does not hold, with the figures either way:
    1  nv12 and i420 on this build equal the parent's medians within the parent's own spread (max - min)
    2  p010 costs no more per booked byte than nv12 on this build; the margin is the nv12 runs' spread
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

Y16_ENTRIES = ("vd_process_yuv420_16", "vd_mosaic_yuv420_16", "vd_smooth_yuv420_16", "vd_yuv420_16_to_rgb",
               "vdt_letterbox_yuv420_16")
PARENT_CASES = ("nv12", "i420")
CASES = ("nv12", "i420", "p010", "p10")
PASSES = ("mosaic", "smooth", "letterbox")
STEP, SURFACES, SCENES = 4, 64, 16


def widen10(t8, shift):
    """int16 words holding the 10-bit values 4 * v + 1 of uint8 samples at `shift` (torch, on the device)."""
    import torch
    x = ((t8.to(torch.int32) * 4 + 1) << shift)
    return torch.where(x >= 32768, x - 65536, x).to(torch.int16)


def one(a):
    """--one parent | this: every case this library has, one context, the same boxes."""
    import torch
    from vdmi import _lib
    parent = a.one == "parent"
    if parent:               # the parent's build does not export the *_yuv420_16 entries
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in Y16_ENTRIES]
    import vdmi
    from nv12bench import nv12_frames
    from yuv420bench import to_i420
    from vdmi import synth, weights
    H, W = 1080, 1920
    dev = torch.device("cuda:0")
    nv = nv12_frames(SCENES, H, W, dev).repeat(SURFACES // SCENES, 1, 1)
    i420 = to_i420(nv, H, W)
    src = {"nv12": nv, "i420": i420}
    if not parent:
        src["p010"] = widen10(nv, 6)
        src["p10"] = widen10(i420, 0)
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=STEP)
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    steps = SURFACES // STEP
    boxes = [vdmi.DeviceBoxes(STEP, 256, dev) for _ in range(steps)]
    rgb = torch.from_numpy(synth.frames(SCENES, H, W, seed=0)).to(dev)
    for s in range(steps):
        sc = (s * STEP) % SCENES
        ctx.process(rgb[sc:sc + STEP], flags=_lib.VD_PROC_FACES, faces=boxes[s])
    ctx.sync()
    del rgb
    out8, out16 = torch.empty_like(nv), torch.empty((SURFACES, H * 3 // 2, W), dtype=torch.int16, device=dev)
    scratch = vdmi.DeviceBoxes(STEP, 256, dev)
    sl = lambda t, s: t[s * STEP:(s + 1) * STEP]
    F = _lib.VD_PROC_FACES

    def calls(case):
        x = src[case]
        if case == "nv12":
            return {"mosaic": lambda s: ctx.mosaic_nv12(sl(x, s), boxes[s], level=a.level, out=sl(out8, s)),
                    "smooth": lambda s: ctx.smooth_nv12(sl(x, s), boxes[s], level=a.level, cells=a.cells, out=sl(out8, s)),
                    "letterbox": lambda s: ctx.process_nv12(sl(x, s), flags=F, faces=scratch)}
        if case == "i420":
            return {"mosaic": lambda s: ctx.mosaic_yuv420(sl(x, s), boxes[s], level=a.level, out=sl(out8, s)),
                    "smooth": lambda s: ctx.smooth_yuv420(sl(x, s), boxes[s], level=a.level, cells=a.cells, out=sl(out8, s)),
                    "letterbox": lambda s: ctx.process_yuv420(sl(x, s), flags=F, faces=scratch)}
        kw = dict(layout="nv12", depth=10, shift=6) if case == "p010" else dict(layout="i420", depth=10, shift=0)
        return {"mosaic": lambda s: ctx.mosaic_yuv420_16(sl(x, s), boxes[s], level=a.level, out=sl(out16, s), **kw),
                "smooth": lambda s: ctx.smooth_yuv420_16(sl(x, s), boxes[s], level=a.level, cells=a.cells, out=sl(out16, s), **kw),
                "letterbox": lambda s: ctx.process_yuv420_16(sl(x, s), flags=F, faces=scratch, **kw)}

    r = {"boxes_per_frame": float(sum(int(b.count.clamp(0, 256).sum()) for b in boxes)) / SURFACES, "cases": {}}
    ctx.timing(True)
    for case in (PARENT_CASES if parent else CASES):
        row = {}
        for name, call in calls(case).items():
            fam = _lib.FAM_LETTERBOX if name == "letterbox" else _lib.FAM_MOSAIC
            for s in range(steps):   # warm-up: one pass
                call(s)
            ctx.sync()
            ctx.timing_reset()
            for _ in range(a.passes):
                for s in range(steps):
                    call(s)
            ctx.sync()
            t, k, work = ctx.timing_read(fam)
            row[name] = {"ms_per_step": round(t / (a.passes * steps), 5), "launches_per_step": k / (a.passes * steps),
                         "bytes_per_step": work / (a.passes * steps)}
        r["cases"][case] = row
    ctx.timing(False)
    ctx.close()
    print("YUV16BENCH " + json.dumps(r), flush=True)


def child(a, which):
    env = dict(os.environ)
    if which == "parent":
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    else:
        env.pop("VDMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--passes", str(a.passes), "--level", str(a.level),
           "--cells", str(a.cells)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("YUV16BENCH "):
            return json.loads(line[len("YUV16BENCH "):])
    raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="passes over the 16 steps behind each figure")
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--cells", type=int, default=16)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", choices=("parent", "this"), help="(internal) one measurement in this process")
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    runs = {"parent": [], "this": []}
    for _ in range(a.repeats):                   # parent, this, parent, this, ...
        for which in ("parent", "this"):
            runs[which].append(child(a, which))  # a failed child raises: nothing more is started
    res = {"what": "family 1 (output pass) and family 2 (face letterbox) per 4-frame step over 64 x 1080p device surfaces "
                   "(16 scenes, four times each) and the face lists of synth's RGB frames: NV12 and I420 by the parent build "
                   "and by this build, P010 and yuv420p10le through the *_yuv420_16 entries by this build; median (min .. max) "
                   "over the runs",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "frame": [1080, 1920], "step_frames": STEP, "surfaces": SURFACES, "level": a.level, "cells": a.cells,
           "repeats": a.repeats, "passes": a.passes, "boxes_per_frame": runs["this"][0]["boxes_per_frame"]}
    e1 = e2 = True
    for p in PASSES:
        row = {}
        ms = lambda which, c: [r["cases"][c][p]["ms_per_step"] for r in runs[which]]
        for c in PARENT_CASES:
            par, cur = stats(ms("parent", c)), stats(ms("this", c))
            spread = round(par["max"] - par["min"], 5)
            ok = abs(cur["median"] - par["median"]) <= spread
            e1 &= ok
            row[c] = {"parent_ms": par, "this_ms": cur, "parent_spread_ms": spread,
                      "this_minus_parent_ms": round(cur["median"] - par["median"], 5), "equal_within_parent_spread": bool(ok)}
        nv = stats(ms("this", "nv12"))
        nb = runs["this"][0]["cases"]["nv12"][p]["bytes_per_step"]
        margin = nv["max"] - nv["min"]
        for c in ("p010", "p10"):
            cur = stats(ms("this", c))
            b = runs["this"][0]["cases"][c][p]["bytes_per_step"]
            per_byte = cur["median"] * nb / b            # ms this case would take at nv12's byte count
            row[c] = {"this_ms": cur, "bytes_per_step": b, "nv12_bytes_per_step": nb, "ratio_to_nv12_ms": round(cur["median"] / nv["median"], 4),
                      "ratio_to_nv12_per_byte": round(per_byte / nv["median"], 4),
                      "launches_per_step": runs["this"][0]["cases"][c][p]["launches_per_step"]}
            if c == "p010":
                ok = per_byte - nv["median"] <= margin
                e2 &= ok
                row[c]["no_more_per_byte_than_nv12"] = bool(ok)
                row[c]["nv12_spread_ms"] = round(margin, 5)
        res[p] = row
    res["expectation_1_8bit_entries_equal_parent"] = "holds" if e1 else "does not hold"
    res["expectation_2_p010_no_more_per_byte_than_nv12"] = "holds" if e2 else "does not hold"
    res["runs"] = runs
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
