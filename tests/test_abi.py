"""The C-ABI library loads on a box without a GPU and exports the symbols include/bodyfit.h declares, and no others."""
import ctypes
import os
import re

import pytest

from bodyfitting_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(REPO, "include", "bodyfit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.SIGNATURES)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built - run __graft_entry__.build()")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), name


def test_library_exports_exactly_the_declared_symbols():
    """host code is compiled with hidden visibility and include/bodyfit.h sets default visibility around its declarations: the
    dynamic bf_* symbols the library defines are the header's, no kernel handle, launcher or bf_host.h helper beside them
    (bf_nearest_stats_read exists only in a -DBF_NEAREST_STATS build, which the product is not)"""
    import shutil
    import subprocess
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built - run __graft_entry__.build()")
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bf_")})
    assert exported == declared_symbols()


def test_no_compute_without_gpu_is_an_error_not_a_fallback(smpl_model, gmm):
    """without a device the product path must fail loudly (no CPU fallback exists)."""
    lib = _lib.load()
    assert lib.bf_version().startswith(b"bodyfit-mi355x")
    if lib.bf_device_count() > 0:
        pytest.skip("a GPU is present")
    from bodyfitting_amd.native import DeviceModel
    with pytest.raises(_lib.BodyfitError):
        DeviceModel(smpl_model, gmm)


def test_missing_library_raises(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libbodyfit.so"))
    with pytest.raises(_lib.BodyfitError):
        _lib.load()


def test_loading_the_library_leaves_the_hardware_queue_setting_alone():
    """csrc/api.hip: how many hardware queues the process's streams share is the host's setting - loading the library (the Python
    binding and the shared object's constructors) neither sets GPU_MAX_HW_QUEUES nor changes the value the user chose"""
    import subprocess
    import sys
    code = ("import ctypes; from bodyfitting_amd import _lib; _lib.load(); "
            "libc = ctypes.CDLL(None); libc.getenv.restype = ctypes.c_char_p; v = libc.getenv(b'GPU_MAX_HW_QUEUES'); "
            "print('unset' if v is None else v.decode())")
    for user_value in (None, "1", "2"):
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        if user_value is not None:
            env["GPU_MAX_HW_QUEUES"] = user_value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
        assert out.returncode == 0, (user_value, out.stderr[-500:])
        assert out.stdout.strip() == (user_value or "unset"), user_value
