"""csrc/lead_state.h, the look-ahead hold's pending-ring bookkeeping shared by the runtime and
the kernel, checked on the host: tools/lead_state_check.cpp (a stand-alone program with its
own main) is compiled with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run against a deque model for every delay in 1..9 and call
sizes 0..12. No Python code runs under a sanitizer, and no GPU is needed."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def _compiler():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def test_lead_state_header_against_the_deque_model(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "lead_state_check"
    src = os.path.join(ROOT, "tools", "lead_state_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lead_state_check: ok" in r.stdout


def test_emission_arithmetic_matches_the_reference_simulator(tmp_path):
    """The header's m = max(0, pending + n - delay) (flush: pending + n), printed by a tiny
    program for a fixed call pattern, equals what tests/lead_ref.py's simulator emits."""
    import lead_ref as lr
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    calls = [(3, 0), (1, 0), (0, 1), (12, 0), (2, 1), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (7, 1)]
    body = "".join(f"m = st.emit({n}, {f}); std::printf(\"%d %d\\n\", m, st.pend); "
                   f"st.end({n}, {f}, VD_LEAD_MODE_PIXELS, 4, 4, 12);\n" for n, f in calls)
    src = tmp_path / "emit.cpp"
    src.write_text('#include "lead_state.h"\n#include <cstdio>\nint main() { LeadState st; st.J = 3; st.motion = 1; '
                   "int m = 0;\n" + body + "return 0; }\n")
    exe = tmp_path / "emit"
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "video-desensitization_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    got = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(calls))]
    s = lr.Stream(10, 10, 3, 30, motion=True)
    want = []
    for n, f in calls:
        pend = s.pending
        b, _ = s.push([[] for _ in range(n)], flush=bool(f))
        want.append((len(b), pend))
    assert got == want
