"""The mode of a pipe's shade launches (wf_launch_mode in csrc/crt_wf_policy.h; driver invariant I11) on the
CPU: tests/host/wf_defer_policy_test.cpp is a stand-alone program over hand-built launch sequences -- which launch may
leave deferred NEE entries, and that the launch behind such a one sweeps the whole pool before tail mode starts.  It is
compiled here for the host alone, with the address and undefined-behaviour sanitizers, and run once; it calls no HIP
function and needs no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "computeraytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_launch_mode_on_hand_built_sequences(tmp_path):
    exe = str(tmp_path / "wf_defer_policy_test")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "--cuda-host-only", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "host", "wf_defer_policy_test.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout
