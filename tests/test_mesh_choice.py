"""Which kernel a mesh pass takes, and in how many launches (bodyfitting_amd/csrc/mesh_choice.h), on the host alone: a stand-alone
program (tests/mesh_choice_main.cpp) built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.
A fit-lane group of calls below 16 frames is one launch of the multi-frame kernel, a lone single-frame SMPL call keeps bf_mesh_kernel,
and calls of 16 frames or more keep a pass each."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(per, G, npf) for npf in (207, 486) for per in (1, 2, 4, 15, 16, 32) for G in (1, 2, 8, 9, 32)]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("mesh_choice") / "mesh_choice")
    # the sanitizers' runtimes linked into the program (clang does so by default): it runs as it is, whatever else the process loads
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    "-Wall", "-Werror", "-I", os.path.join(REPO, "bodyfitting_amd", "csrc"), os.path.join(REPO, "tests", "mesh_choice_main.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_program_ran_clean(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-4000:]
    assert report.stderr.strip() == "", report.stderr[-4000:]
    assert len([ln for ln in report.stdout.splitlines() if ln.startswith("ok ")]) == len(CASES)


@pytest.mark.parametrize("per,G,npf", CASES)
def test_group_is_one_multi_launch_and_large_calls_keep_their_pass(report, per, G, npf):
    assert f"ok {per} {G} {npf}" in report.stdout.splitlines(), report.stdout[-2000:] + report.stderr[-2000:]
