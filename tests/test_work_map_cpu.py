"""The region-major work shards (csrc/crt_work_map.h, option "wf_affinity") on the CPU: tests/host/work_map_test.cpp is a
stand-alone program that enumerates the mapping local chunk -> (sample, tile) for 1, 5, 7, 8, 9, 45 and 32 400 tiles times
1, 3, 8, 13 and 64 samples and checks that it is a partition of the batch's work.  It is compiled here for the host alone,
with the address and undefined-behaviour sanitizers, and run once; it includes no HIP header and needs no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "computeraytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_work_map_is_a_partition(tmp_path):
    exe = str(tmp_path / "work_map_test")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "--cuda-host-only", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "host", "work_map_test.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout
