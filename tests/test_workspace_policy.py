"""When a device-route workspace allocates and when a call waits for the one before it (bodyfitting_amd/csrc/workspace_policy.h), on
the host alone: a stand-alone program (tests/workspace_policy_main.cpp) built with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run once.  A loop of a model's forward and reverse calls allocates in its first round only, slots only
grow, and only a call on another stream than its predecessor's waits."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPERTIES = ("settles", "grow_only", "rounding", "failed_growth", "stream_switch")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("workspace_policy") / "workspace_policy")
    # the sanitizers' runtimes linked into the program (clang does so by default): it runs as it is, whatever else the process loads
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    "-Wall", "-Werror", "-I", os.path.join(REPO, "bodyfitting_amd", "csrc"), os.path.join(REPO, "tests", "workspace_policy_main.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_program_ran_clean(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-4000:]
    assert report.stderr.strip() == "", report.stderr[-4000:]


@pytest.mark.parametrize("name", PROPERTIES)
def test_property(report, name):
    assert f"ok {name}" in report.stdout.splitlines(), report.stdout[-2000:] + report.stderr[-2000:]
