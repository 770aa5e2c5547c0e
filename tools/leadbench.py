"""Cost of the look-ahead hold at the bench shape: Context.process_lead at lead=2 on 64
synthetic 1080p frames already in HBM (fp32, faces | plates | mosaic, as bench.py's flagship
step), against Context.process on the PARENT commit's build, both in one session.

    python tools/leadbench.py --parent-lib PATH/libvdmi.so [--steps 20] [--warmup 3]
                              [--repeats 3] [--json profiles/lead_1080p.json]

Every measurement is a child process of its own (a fresh context, a fresh library: the parent's
build is loaded through VDMI_LIB, where the entry points it lacks are simply not bound), the two
builds alternating, `--repeats` of each. Per run: ms/step in the steady state -- warm-up first,
which also fills the pending ring, then the steps ended by one synchronise; from then on every
process_lead call pushes 64 frames and emits 64. The added work per step is one list launch
(timing family 3) and the device-to-device copy of the `delay` frames that stay pending
(family 4: 2 x delay x 6.2 MB read and written at 1080p), so the step should sit inside the
parent's own repeat spread plus that copy. The seeded noise frames share nothing from one frame
to the next, so nearly every box of the next `lead` frames is led: the heavy case for the list
kernel and for the mosaic behind it (a video leads a box only before a first detection).

With --format the tool measures the look-ahead hold on video surfaces instead (the two builds still
alternating in one session):

    python tools/leadbench.py --format all --parent-lib PATH/libvdmi.so [--leads 2,8] [--passes 3]
                              [--repeats 3] [--json profiles/lead_yuv420_1080p.json]

64 synthetic 1080p surfaces already in HBM are pushed in 4-frame steps (fp32, faces | plates | mosaic,
max_batch 4) at every lead of --leads, with pixelation and with the scaled smooth blur, in the formats
named: nv12 (through process_lead_nv12), nv12_new (NV12 through process_lead_yuv420), i420, nv21, p010,
yuv420p10le. A child process per build and repeat walks every case with a fresh context each; the
parent's build runs NV12 alone (lead off and process_lead_nv12). Per case: ms per step, the ring's
bytes, the ring update (timing family 4, the lead-off context's share subtracted) and what the lead
adds over the same build's context with lead = 0. The result line states whether NV12 through either
entry equals the parent's within the run-to-run spread of the repeats, and how far each push lands
from a copy of the same bytes at the HBM copy rate.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))

LEAD_ENTRIES = ("vd_lead", "vd_lead_pending", "vd_process_lead", "vd_lead_lists", "vd_read_lead")


def one(a):
    """A single measurement in this process: --one base (process) or --one lead (process_lead)."""
    import torch
    from vdmi import _lib
    if a.one == "base":      # the parent's build does not export the lead entry points
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in LEAD_ENTRIES]
    import vdmi
    from vdmi import synth, weights
    B, H, W = a.batch, 1080, 1920
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synth.frames(B, H, W, seed=0)).to(dev)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    lead = a.lead if a.one == "lead" else 0
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=B, **({"lead": lead} if lead else {}))
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    ctx.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
    faces, plates = vdmi.DeviceBoxes(B, 256, dev), vdmi.DeviceBoxes(B, 256, dev)
    out = torch.empty((B + lead, H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    emitted = []
    if lead:
        def step():
            emitted.append(len(ctx.process_lead(frames, out, faces=faces, plates=plates, flags=flags)[0]))
    else:
        def step():
            ctx.process(frames, out, faces=faces, plates=plates, flags=flags)
    for _ in range(max(a.warmup, 1)):
        step()
    ctx.sync()
    del emitted[:]
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
         "faces_per_frame": float(faces.count.float().mean().item())}
    if lead:
        assert emitted == [B] * a.steps, emitted          # the steady state: 64 in, 64 out
        r["led_per_frame"] = float(ctx.read_lead(B, "lead", cap=1).count.mean())
    # families 3 (post: decode, NMS, the list launch) and 4 (other: the ring copy among them) in
    # steps of their own (events around every launch slow the step); the lead run's figures minus
    # the parent's are the list launch and the copy
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(a.post_steps):
        step()
    for fam, key in ((_lib.FAM_POST, "post"), (_lib.FAM_OTHER, "other")):
        t, launches, _ = ctx.timing_read(fam)
        r[f"{key}_ms_per_step"] = round(t / a.post_steps, 4)
        r[f"{key}_launches_per_step"] = launches / a.post_steps
    ctx.timing(False)
    ctx.close()
    print("LEADBENCH " + json.dumps(r), flush=True)


# ---- surfaces (--format) ---------------------------------------------------------------------------
FORMATS = ("nv12", "nv12_new", "i420", "nv21", "p010", "yuv420p10le")
SURFACE_MODES = {"pixelate": {}, "smooth": {"blur": "gaussian", "cells": 8}}
NEW_ENTRIES = ("vd_process_lead_yuv420", "vd_process_lead_yuv420_16")
SN, SSTEP, SH, SW = 64, 4, 1080, 1920
HBM_COPY_BYTES_PER_MS = 6.3e9            # the measured float4-copy rate of the part, read + written bytes


def surface_frames(fmt, nv):
    """The 64 NV12 bench surfaces in `fmt`: the same samples re-laid, widened to 10 bits for the 16-bit formats."""
    import torch
    if fmt in ("nv12", "nv12_new"):
        return nv
    y, c = nv[:, :SH], nv[:, SH:].reshape(SN, SH // 2, SW // 2, 2)
    if fmt in ("nv21", "p010"):
        pairs = c.flip(-1) if fmt == "nv21" else c
        f = torch.cat([y, pairs.reshape(SN, SH // 2, SW)], 1).contiguous()
        return f if fmt == "nv21" else (f.to(torch.int32) << 8).to(torch.int16)      # value << 2 at shift 6
    f = torch.cat([y.reshape(SN, -1), c[..., 0].reshape(SN, -1), c[..., 1].reshape(SN, -1)], 1).reshape(SN, SH * 3 // 2, SW)
    return f.contiguous() if fmt == "i420" else (f.to(torch.int16) << 2)


def surface_calls(ctx, fmt, lead):
    """(the call of a step, keyword arguments) for surfaces of `fmt`, with the look-ahead or without."""
    if fmt == "nv12":
        return (ctx.process_lead_nv12 if lead else ctx.process_nv12), {}
    if fmt in ("p010", "yuv420p10le"):
        kw = dict(layout="nv12" if fmt == "p010" else "i420", depth=10)
        return (ctx.process_lead_yuv420_16 if lead else ctx.process_yuv420_16), kw
    kw = dict(layout={"nv12_new": "nv12"}.get(fmt, fmt))
    return (ctx.process_lead_yuv420 if lead else ctx.process_yuv420), kw


def one_surfaces(a):
    """Every case of one build in this process, a fresh context each: {"mode/fmt/J": figures}."""
    import torch
    from vdmi import _lib
    parent = a.one_surfaces == "parent"
    if parent:
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRIES]
    import vdmi
    from vdmi import weights
    dev = torch.device("cuda:0")
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    leads = [int(v) for v in a.leads.split(",")]
    formats = ["nv12"] if parent else a.format.split(",")
    k = SN // SSTEP
    res = {}
    from nv12bench import nv12_frames
    nv = nv12_frames(SN, SH, SW, dev)
    for fmt in formats:
        src = surface_frames(fmt, nv)
        for mode in sorted(SURFACE_MODES):
            for lead in [0] + leads:
                if lead == 0 and fmt == "nv12_new":
                    continue                          # lead off is the format's own process call: nv12's
                ctx = vdmi.Context(device=0, precision="fp32", max_batch=SSTEP, lead=lead, **SURFACE_MODES[mode])
                ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
                ctx.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
                faces, plates = vdmi.DeviceBoxes(SSTEP, 256, dev), vdmi.DeviceBoxes(SSTEP, 256, dev)
                out = torch.empty((SSTEP + ctx.lead_delay,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
                call, kw = surface_calls(ctx, fmt, lead)
                emitted = []

                def sweep():
                    for lo in range(0, SN, SSTEP):
                        o = call(src[lo:lo + SSTEP], out if lead else out[:SSTEP], faces=faces, plates=plates, flags=flags, **kw)[0]
                        emitted.append(len(o))

                sweep()                               # warm-up: allocations, and the ring fills
                ctx.sync()
                del emitted[:]
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    sweep()
                ctx.sync()
                steps = a.passes * k
                r = {"ms_per_step": round((time.perf_counter() - t0) * 1e3 / steps, 4)}
                assert emitted == [SSTEP] * steps, emitted
                ctx.timing(True)
                ctx.timing_reset()
                sweep()
                ctx.sync()
                t, launches, work = ctx.timing_read(_lib.FAM_OTHER)
                r.update(ring_ms_per_step=round(t / k, 5), ring_launches_per_step=launches / k, ring_bytes_per_step=work / k)
                ctx.timing(False)
                if lead:
                    r["ring_bytes"] = int(ctx.lead_delay * SH * SW * 3 // 2 * src.element_size())
                    ctx.hold_reset()
                ctx.close()
                res[f"{mode}/{fmt}/J{lead}"] = r
        del src
    print("LEADBENCH " + json.dumps(res), flush=True)


def surfaces_main(a):
    fmts = list(FORMATS) if a.format == "all" else a.format.split(",")
    for f in fmts:
        if f not in FORMATS:
            raise SystemExit(f"--format {f}: expected 'all' or a list of {FORMATS}")
    a.format = ",".join(fmts)
    leads = [int(v) for v in a.leads.split(",")]
    runs = {"parent": [], "this": []}
    for _ in range(a.repeats):                        # parent, this, parent, this, ...: a failed child raises
        for which in ("parent", "this"):
            env = dict(os.environ)
            if which == "parent":
                env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("VDMI_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--one-surfaces", which, "--format", a.format, "--leads", a.leads,
                   "--passes", str(a.passes)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:
                raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("LEADBENCH ")]
            if not line:
                raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")
            runs[which].append(json.loads(line[-1][len("LEADBENCH "):]))

    def vals(which, key, field="ms_per_step"):
        return [r[key][field] for r in runs[which]]

    def mean(v):
        return sum(v) / len(v)

    cases = {}
    for mode in sorted(SURFACE_MODES):
        for fmt in fmts:
            off_key = f"{mode}/{'nv12' if fmt == 'nv12_new' else fmt}/J0"
            for J in leads:
                key = f"{mode}/{fmt}/J{J}"
                ms, off = vals("this", key), vals("this", off_key)
                ring = mean(vals("this", key, "ring_ms_per_step")) - mean(vals("this", off_key, "ring_ms_per_step"))
                nbytes = mean(vals("this", key, "ring_bytes_per_step"))
                c = {"lead_ms_per_step": round(mean(ms), 4), "off_ms_per_step": round(mean(off), 4),
                     "lead_added_ms": round(mean(ms) - mean(off), 4),
                     "spread_ms": round(max(max(ms) - min(ms), max(off) - min(off)), 4),
                     "ring_bytes": runs["this"][0][key]["ring_bytes"], "ring_bytes_per_step": nbytes,
                     "ring_ms_per_step": round(ring, 5),
                     "ring_launches_per_step": mean(vals("this", key, "ring_launches_per_step")) -
                     mean(vals("this", off_key, "ring_launches_per_step")),
                     "ring_ms_at_hbm_copy_rate": round(nbytes / HBM_COPY_BYTES_PER_MS, 5)}
                c["ring_times_the_hbm_copy"] = round(ring / c["ring_ms_at_hbm_copy_rate"], 2) if nbytes else None
                if fmt in ("nv12", "nv12_new"):       # against the parent's process_lead_nv12
                    pk = f"{mode}/nv12/J{J}"
                    pm = vals("parent", pk)
                    spread = max(max(pm) - min(pm), max(ms) - min(ms))
                    c.update(parent_lead_ms_per_step=round(mean(pm), 4), parent_runs_ms=pm, this_runs_ms=ms,
                             difference_ms=round(mean(ms) - mean(pm), 4), run_to_run_spread_ms=round(spread, 4),
                             equals_parent_within_spread=bool(abs(mean(ms) - mean(pm)) <= spread),
                             parent_ring_ms_per_step=round(mean(vals("parent", pk, "ring_ms_per_step")) -
                                                           mean(vals("parent", f"{mode}/nv12/J0", "ring_ms_per_step")), 5))
                cases[key] = c
    res = {"what": "look-ahead hold on 4:2:0 surfaces by format: process_lead_nv12 / process_lead_yuv420 / "
                   "process_lead_yuv420_16 against the same build with lead = 0, NV12 also against the parent commit's "
                   "process_lead_nv12",
           "machine": "one MI355X, the two builds alternating in one session, a process per build and repeat",
           "frames": SN, "step": SSTEP, "frame": [SH, SW], "precision": "fp32", "passes": a.passes, "repeats": a.repeats,
           "note": "ms per 4-frame step; ring_* is timing family 4 from an event-timed pass of its own, the lead-off "
                   "context's share subtracted; ring_ms_at_hbm_copy_rate: the ring's bytes read + written at 6.3 TB/s",
           "cases": cases, "runs": runs}
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


def child(a, which):
    env = dict(os.environ)
    if which == "base":
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    else:
        env.pop("VDMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", which, "--steps", str(a.steps), "--warmup",
           str(a.warmup), "--batch", str(a.batch), "--lead", str(a.lead), "--post-steps", str(a.post_steps)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{which} run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("LEADBENCH "):
            return json.loads(line[len("LEADBENCH "):])
    raise RuntimeError(f"{which} run printed no result:\n{p.stdout[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lead", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--post-steps", type=int, default=5, help="event-timed steps behind the family figures")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", choices=("base", "lead"), help="(internal) one measurement in this process")
    ap.add_argument("--json", help="also write the result line to this file")
    ap.add_argument("--format", help="measure surfaces instead: 'all' or a comma list of " + ", ".join(FORMATS))
    ap.add_argument("--leads", default="2,8", help="(--format) the leads measured")
    ap.add_argument("--passes", type=int, default=3, help="(--format) timed passes over the 64 surfaces (16 steps each)")
    ap.add_argument("--one-surfaces", choices=("parent", "this"), help="(internal) every surface case of one build")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if a.one_surfaces:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        return one_surfaces(a)
    if a.format:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
        if a.child_timeout == 240:
            a.child_timeout = 900
        return surfaces_main(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    runs = {"base": [], "lead": []}
    for _ in range(a.repeats):                   # parent, this, parent, this, ...
        for which in ("base", "lead"):
            runs[which].append(child(a, which))  # a failed child raises: nothing more is started
    pm = [r["ms_per_step"] for r in runs["base"]]
    lm = [r["ms_per_step"] for r in runs["lead"]]
    delay = a.lead
    frame_mb = 1080 * 1920 * 3 / 1e6
    res = {"what": f"look-ahead hold: process_lead at lead={a.lead} vs process on the parent commit's build",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "batch": a.batch, "frame": [1080, 1920], "precision": "fp32", "steps": a.steps, "warmup": a.warmup,
           "note": "noise frames: nearly every box of the next `lead` frames is led (heavy case)",
           "parent_process_ms_per_step": pm, "lead_process_lead_ms_per_step": lm,
           "parent_mean": round(sum(pm) / len(pm), 3), "lead_mean": round(sum(lm) / len(lm), 3),
           "difference_ms": round(sum(lm) / len(lm) - sum(pm) / len(pm), 3),
           "parent_spread_ms": round(max(pm) - min(pm), 3),
           "derived_ring_copy_mb_per_step": round(2 * delay * frame_mb, 1),
           "list_launch_ms": round(sum(r["post_ms_per_step"] for r in runs["lead"]) / len(lm)
                                   - sum(r["post_ms_per_step"] for r in runs["base"]) / len(pm), 4),
           "ring_copy_ms": round(sum(r["other_ms_per_step"] for r in runs["lead"]) / len(lm)
                                 - sum(r["other_ms_per_step"] for r in runs["base"]) / len(pm), 4),
           "lead_runs": runs["lead"], "parent_runs": runs["base"]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
