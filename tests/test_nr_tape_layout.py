"""Where a device-route tape's buffers lie in the tensor it borrows (bodyfitting_amd/csrc/nr_tape_layout.h), on the host alone: a
stand-alone program (tests/nr_tape_layout_main.cpp) built with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run once - no library is loaded into Python for it.  Segments do not overlap, every offset is a
multiple of 256 bytes, absent segments have size 0, totals do not overflow size_t, and every size is what the host route's
allocations are for the same render.  The exported bf_nr_tape_layout is the same function: checked against the header's numbers
where the library is built."""
import ctypes
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPERTIES = ("sweep", "refusals")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("nr_tape_layout") / "nr_tape_layout")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    "-Wall", "-Werror", "-I", os.path.join(REPO, "bodyfitting_amd", "csrc"), os.path.join(REPO, "tests", "nr_tape_layout_main.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_program_ran_clean(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-4000:]
    assert report.stderr.strip() == "", report.stderr[-4000:]


@pytest.mark.parametrize("name", PROPERTIES)
def test_property(report, name):
    assert any(line.startswith(f"ok {name}") for line in report.stdout.splitlines()), report.stdout[-2000:] + report.stderr[-2000:]


def test_the_header_holds_no_hip_and_the_library_exports_the_same_function():
    text = open(os.path.join(REPO, "bodyfitting_amd", "csrc", "nr_tape_layout.h")).read()
    assert [line for line in text.splitlines() if line.startswith("#include")] == ["#include <cstddef>"] and "__global__" not in text
    from bodyfitting_amd import _lib, native
    assert "bf_nr_tape_layout" in _lib.SIGNATURES and "int bf_nr_tape_layout(" in open(os.path.join(REPO, "include", "bodyfit.h")).read()
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built - run __graft_entry__.build()")
    # is 64, 27552 records, 6890 vertices, lit, both tape flags, rgb, a directional light: every segment present
    got = native.nr_tape_layout(64, 27552, 6890, True, 3, True, True)
    sizes = dict(view=22, pix=64 * 64 * 5, frec=27552 * 20, light=27552 * 3, verts=6890 * 3, pv=6890 * 3, rgbmap=64 * 64 * 3, unlit=64 * 64 * 3)
    assert got["sizes"] == sizes
    at = 0
    for name in native.NR_TAPE_SEGMENTS:
        assert got["offsets"][name] == at and at % 64 == 0
        at += -(-sizes[name] // 64) * 64
    assert got["total"] == at
    # no tape (flags 0), unlit, no rgb: the view, the pixel map and the records alone
    bare = native.nr_tape_layout(16, 5, 3, False, 0, False, True)
    assert [k for k, v in bare["sizes"].items() if v] == ["view", "pix", "frec"] and bare["total"] == 64 + 1280 + 128
    out = (ctypes.c_uint64 * 17)()
    assert _lib.load().bf_nr_tape_layout(0, 1, 1, 0, 0, 0, 0, out) == -1 and _lib.load().bf_nr_tape_layout(16, 1, 1, 0, 0, 0, 0, None) == -1
