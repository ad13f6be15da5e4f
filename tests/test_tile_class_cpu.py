"""The tile classifier (csrc/crt_tile_class.h) on the CPU: tests/host/tile_class_test.cpp is a stand-alone
program that classifies every tile of hand-made root nodes and cameras with the header's interval forms and checks the
MISS and ENTER tiles against the header's scalar functions by brute force.  It is compiled here for the host alone, with
the address and undefined-behaviour sanitizers and the library's floating-point flags, and run once; it calls no HIP
function and needs no GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "computeraytracer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_tile_classes_against_brute_force(tmp_path):
    exe = str(tmp_path / "tile_class_test")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "--cuda-host-only", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "tile_class_test.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failed" in run.stdout
