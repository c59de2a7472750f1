"""Slot arithmetic and packing of a fit lane's input arena (bodyfitting_amd/csrc/lane_slots.h) on the host alone: a stand-alone
program (tests/lane_pack_main.cpp) built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.
Filling slot s writes exactly that slot's three ranges with what the single-call packing produces, and the ranges a group's one
transfer moves are exactly slots [0, G + staged)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(F, V, W, n_params) for F in (1, 4, 16) for V in (1, 5, 12, 50) for W in (1, 3, 8) for n_params in (86, 87)]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lane_pack") / "lane_pack")
    # the sanitizers' runtimes linked into the program (clang does so by default): it runs as it is, whatever else the process loads
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    "-Wall", "-Werror", "-I", os.path.join(REPO, "bodyfitting_amd", "csrc"), os.path.join(REPO, "tests", "lane_pack_main.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_program_ran_clean(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-4000:]
    assert report.stderr.strip() == "", report.stderr[-4000:]
    assert len([ln for ln in report.stdout.splitlines() if ln.startswith("ok ")]) == len(CASES)


@pytest.mark.parametrize("F,V,W,n_params", CASES)
def test_slot_is_packed_alone_and_prefix_ranges_cover_the_group(report, F, V, W, n_params):
    assert f"ok {F} {V} {W} {n_params}" in report.stdout.splitlines(), report.stdout[-2000:] + report.stderr[-2000:]
