"""Cost of the look-ahead hold on NV12 surfaces: Context.process_lead_nv12 over 64 synthetic 1080p
surfaces already in HBM, pushed in 4-frame steps (fp32, faces | plates | mosaic, max_batch 4: a
decoder's cadence), at lead J in {2, 8}, for pixelation and for the scaled smooth blur
(blur="gaussian", cells=8). Beside it, from the PARENT commit's build in the same session:

    nv12_off   Context.process_nv12 with lead off            (what the NV12 lead adds its cost to)
    rgb_off    Context.process on nv12_to_rgb of the frames  (what the RGB lead adds its cost to)
    rgb_lead   Context.process_lead at the same J on them

and, informational, this build's process_nv12 with lead off (nv12_off_this), which tells a difference
between the two builds from the cost of the lead.

    python tools/leadnv12bench.py --parent-lib PATH/libvdmi.so [--passes 3] [--repeats 3]
                                  [--json profiles/lead_nv12_1080p.json]

Every measurement is a child process of its own (a fresh context and library; the parent's build is
loaded through VDMI_LIB with the entry point it lacks not bound), the kinds alternating, `--repeats`
of each. Per run: one warm-up pass over the 64 frames (it fills the ring), then `--passes` passes
ended by one synchronise -> ms per 4-frame step; then one event-timed pass for the timing families,
family 4 among them (the ring: RGB device-to-device copies, NV12 the slot moves and the one push
launch per step) with its bytes. The expectation the result line answers, with the parent's own
repeat spread beside it: the NV12 lead's added cost over nv12_off is not above the RGB lead's added
cost over rgb_off (it moves half the ring bytes)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-desensitization_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_ENTRIES = ("vd_process_lead_nv12",)
PARENT_KINDS = ("nv12_off", "rgb_off", "rgb_lead")            # measured on the parent's build
KINDS = PARENT_KINDS + ("nv12_off_this", "nv12_lead")         # this build: process_nv12 lead off (informational), the lead
MODES = {"pixelate": {}, "smooth": {"blur": "gaussian", "cells": 8}}
N, STEP, H, W = 64, 4, 1080, 1920


def one(a):
    """A single measurement in this process."""
    import torch
    from vdmi import _lib
    if a.one in PARENT_KINDS:
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRIES]
    import vdmi
    from vdmi import weights
    from nv12bench import nv12_frames
    dev = torch.device("cuda:0")
    nv = nv12_frames(N, H, W, dev)
    rgb = None
    if a.one.startswith("rgb"):
        rgb = torch.from_numpy(vdmi.nv12_to_rgb(nv.cpu().numpy())).to(dev)
        del nv
    lead = a.lead if a.one.endswith("lead") else 0
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC
    ctx = vdmi.Context(device=0, precision="fp32", max_batch=STEP, lead=lead, **MODES[a.mode])
    ctx.load_weights(_lib.VD_NET_RETINAFACE, weights.retinaface_state_dict(0))
    ctx.load_weights(_lib.VD_NET_YOLOV8N, weights.yolov8n_state_dict(0))
    faces, plates = vdmi.DeviceBoxes(STEP, 256, dev), vdmi.DeviceBoxes(STEP, 256, dev)
    src = rgb if rgb is not None else nv
    out = torch.empty((STEP + lead,) + tuple(src.shape[1:]), dtype=torch.uint8, device=dev)
    call = {"nv12_off": ctx.process_nv12, "nv12_off_this": ctx.process_nv12, "rgb_off": ctx.process,
            "rgb_lead": ctx.process_lead, "nv12_lead": getattr(ctx, "process_lead_nv12", None)}[a.one]
    emitted = []

    def sweep():
        for lo in range(0, N, STEP):
            o = call(src[lo:lo + STEP], out if lead else out[:STEP], faces=faces, plates=plates, flags=flags)[0]
            emitted.append(len(o))

    sweep()                                        # warm-up: allocations, and the ring fills
    ctx.sync()
    del emitted[:]
    t0 = time.perf_counter()
    for _ in range(a.passes):
        sweep()
    ctx.sync()
    steps = a.passes * (N // STEP)
    r = {"ms_per_step": round((time.perf_counter() - t0) * 1e3 / steps, 4)}
    assert emitted == [STEP] * steps, emitted      # the steady state: 4 in, 4 out
    if lead:
        r["led_per_frame"] = float(ctx.read_lead(STEP, "lead", cap=1).count.mean())
    ctx.timing(True)
    ctx.timing_reset()
    sweep()
    ctx.sync()
    t, launches, work = ctx.timing_read(_lib.FAM_OTHER)
    k = N // STEP
    r.update(ring_ms_per_step=round(t / k, 5), ring_launches_per_step=launches / k, ring_bytes_per_step=work / k)
    fams = [ctx.timing_read(f) for f in range(7)]  # conv, output pass, letterbox, post + lists, other + ring, plate conv, cells
    r.update(family_ms_per_step=[round(f[0] / k, 5) for f in fams], family_launches_per_step=[f[1] / k for f in fams])
    ctx.timing(False)
    if lead:
        r["ring_bytes"] = int(ctx.lead_delay * H * W * (1.5 if a.one == "nv12_lead" else 3))
        ctx.hold_reset()
    ctx.close()
    print("LEADNV12BENCH " + json.dumps(r), flush=True)


def child(a, kind, mode, lead):
    env = dict(os.environ)
    if kind not in PARENT_KINDS:
        env.pop("VDMI_LIB", None)
    else:
        env["VDMI_LIB"] = os.path.abspath(a.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--mode", mode, "--lead", str(lead), "--passes",
           str(a.passes)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{kind} {mode} J={lead} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("LEADNV12BENCH "):
            return json.loads(line[len("LEADNV12BENCH "):])
    raise RuntimeError(f"{kind} run printed no result:\n{p.stdout[-2000:]}")


def _mean(runs, key="ms_per_step"):
    return sum(r[key] for r in runs) / len(runs)


def _fam_diff(runs, base):
    return [round(_mean([{"v": r["family_ms_per_step"][f]} for r in runs], "v") -
                  _mean([{"v": r["family_ms_per_step"][f]} for r in base], "v"), 5) for f in range(7)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libvdmi.so built from the parent commit")
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the 64 frames (16 steps each)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leads", default="2,8")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", choices=KINDS, help="(internal) one measurement in this process")
    ap.add_argument("--mode", choices=sorted(MODES), default="pixelate")
    ap.add_argument("--lead", type=int, default=2)
    ap.add_argument("--json", help="also write the result line to this file")
    a = ap.parse_args()
    if a.one:
        return one(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's libvdmi.so is needed for the comparison")
    leads = [int(v) for v in a.leads.split(",")]
    runs = {}
    for _ in range(a.repeats):                      # a failed child raises: nothing more is started
        for mode in sorted(MODES):
            for kind in KINDS:
                for J in (leads if kind.endswith("lead") else [0]):
                    runs.setdefault(f"{mode}/{kind}/J{J}", []).append(child(a, kind, mode, J))
    cases = {}
    for mode in sorted(MODES):
        noff, roff = runs[f"{mode}/nv12_off/J0"], runs[f"{mode}/rgb_off/J0"]
        spread = max(max(r["ms_per_step"] for r in x) - min(r["ms_per_step"] for r in x) for x in (noff, roff))
        for J in leads:
            nl, rl = runs[f"{mode}/nv12_lead/J{J}"], runs[f"{mode}/rgb_lead/J{J}"]
            spread_j = max(spread, max(r["ms_per_step"] for r in rl) - min(r["ms_per_step"] for r in rl))
            nv_added, rgb_added = _mean(nl) - _mean(noff), _mean(rl) - _mean(roff)
            cases[f"{mode}/J{J}"] = {
                "nv12_lead_ms_per_step": round(_mean(nl), 4), "parent_nv12_off_ms_per_step": round(_mean(noff), 4),
                "parent_rgb_lead_ms_per_step": round(_mean(rl), 4), "parent_rgb_off_ms_per_step": round(_mean(roff), 4),
                "this_nv12_off_ms_per_step": round(_mean(runs[f"{mode}/nv12_off_this/J0"]), 4),   # informational
                "nv12_lead_added_ms": round(nv_added, 4), "rgb_lead_added_ms": round(rgb_added, 4),
                "parent_spread_ms": round(spread_j, 4),
                "nv12_added_not_above_rgb_added_within_spread": bool(nv_added <= rgb_added + spread_j),
                # family 4 also times a few launches of the nets (work 0): the lead-off run's share is subtracted
                "nv12_ring_ms_per_step": round(_mean(nl, "ring_ms_per_step") - _mean(noff, "ring_ms_per_step"), 5),
                "rgb_ring_ms_per_step": round(_mean(rl, "ring_ms_per_step") - _mean(roff, "ring_ms_per_step"), 5),
                "nv12_ring_launches_per_step": _mean(nl, "ring_launches_per_step") - _mean(noff, "ring_launches_per_step"),
                "nv12_ring_bytes_per_step": _mean(nl, "ring_bytes_per_step"),
                "rgb_ring_bytes_per_step": _mean(rl, "ring_bytes_per_step"),
                "nv12_ring_bytes": nl[0]["ring_bytes"], "rgb_ring_bytes": rl[0]["ring_bytes"],
                # event-timed families 0..6, ms per step, means over the repeats: what each lead adds, family by family
                "nv12_lead_added_family_ms": _fam_diff(nl, noff), "rgb_lead_added_family_ms": _fam_diff(rl, roff)}
    res = {"what": "look-ahead hold on NV12 surfaces: process_lead_nv12 vs the parent commit's process_nv12 (lead off), "
                   "and the parent's RGB process_lead vs process on the converted frames",
           "machine": "one MI355X, the runs alternating in one session, a process each",
           "frames": N, "step": STEP, "frame": [H, W], "precision": "fp32", "passes": a.passes, "repeats": a.repeats,
           "note": "ms per 4-frame step; ring_* is timing family 4 from an event-timed pass of its own; "
                   "parent_spread_ms: the largest max - min over the parent's repeats of the kinds compared",
           "cases": cases, "runs": runs}
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
