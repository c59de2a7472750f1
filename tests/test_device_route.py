"""Which route a call of the torch drop-ins takes (bodyfitting_amd/_autograd.py: route_for), on the CPU: the device route only when
one is offered, the switch is on, torch and the library share a HIP runtime, and every input that is present is a float32 tensor on
the offering object's GPU.  Everything else - and that includes a GPU user whose process loaded the library before torch - takes
the host route, and nothing raises.  Tensors of a GPU do not exist here: stand-ins with a tensor's `device` and `dtype` do."""
import itertools
import types

import numpy as np
import pytest
import torch

from bodyfitting_amd import _autograd


def fake(device="cuda:0", dtype=torch.float32):
    return types.SimpleNamespace(device=torch.device(device), dtype=dtype)


ON_GPU0 = [fake(), fake(), fake()]


def test_truth_table_of_the_conditions():
    """every combination of (route offered, switch, shared runtime, inputs that qualify): "device" for the one row where all hold"""
    for offered, enabled, shared, qualify in itertools.product((True, False), repeat=4):
        inputs = ON_GPU0 if qualify else [fake(), torch.zeros(3), fake()]
        got = _autograd.route_for(inputs, 0 if offered else None, enabled, shared)
        assert got == ("device" if offered and enabled and shared and qualify else "host"), (offered, enabled, shared, qualify)


@pytest.mark.parametrize("name,inputs", [
    ("cpu tensors", [torch.zeros(2, 10), torch.zeros(2, 3)]),
    ("one cpu tensor among gpu ones", [fake(), torch.zeros(2, 3), fake()]),
    ("mixed gpus", [fake("cuda:0"), fake("cuda:1")]),
    ("another gpu than the model's", [fake("cuda:1"), fake("cuda:1")]),
    ("a gpu without an index", [fake("cuda")]),
    ("float64", [fake(), fake(dtype=torch.float64)]),
    ("float16", [fake(dtype=torch.float16)]),
    ("numpy", [np.zeros((2, 10), np.float32)]),
    ("nothing present", [None, None]),
    ("no inputs", []),
])
def test_inputs_that_take_the_host_route(name, inputs):
    assert _autograd.route_for(inputs, 0, True, True) == "host", name


def test_an_argument_not_passed_does_not_decide():
    assert _autograd.route_for([fake(), None, fake(), None], 0, True, True) == "device"
    assert _autograd.route_for([None, fake("cuda:2")], 2, True, True) == "device"
    assert _autograd.route_for([None, torch.zeros(1)], 0, True, True) == "host"


def test_the_switch_and_the_runtime_each_veto():
    assert _autograd.route_for(ON_GPU0, 0, True, True) == "device"
    assert _autograd.route_for(ON_GPU0, 0, False, True) == "host"            # BF_TORCH_DEVICE_ROUTE=0
    assert _autograd.route_for(ON_GPU0, 0, True, False) == "host"            # two HIP runtimes in the process
    assert _autograd.route_for(ON_GPU0, None, True, True) == "host"          # a drop-in that offers no device route


def test_cpu_tensors_never_ask_the_library_about_the_runtime(monkeypatch):
    """the pointer check is for GPU tensors alone: a CPU call decides without loading anything"""
    def boom(*a):
        raise AssertionError("asked")
    monkeypatch.setattr(_autograd, "shares_runtime", boom)
    offer = types.SimpleNamespace(device=0)
    assert _autograd.chosen_route([torch.zeros(2, 3, requires_grad=True)], offer) == "host"
    assert _autograd.chosen_route([torch.zeros(2, 3)], None) == "host"


def test_the_runtime_is_asked_once_per_gpu(monkeypatch, capsys):
    from bodyfitting_amd import native
    asked = []
    monkeypatch.setattr(native, "device_pointer_check", lambda device, address: asked.append((device, address)) or False)
    monkeypatch.setattr(_autograd, "_SHARED", {})
    assert _autograd.shares_runtime(0, 4096) is False and _autograd.shares_runtime(0, 8192) is False
    assert asked == [(0, 4096)]
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "import torch first" in err          # one line, naming the import order
    monkeypatch.setattr(native, "device_pointer_check", lambda device, address: True)
    assert _autograd.shares_runtime(1, 4096) is True and capsys.readouterr().err == ""


def test_the_switch_is_read_from_the_environment(monkeypatch):
    for value, want in (("0", False), ("1", True), (None, True), (" 0 ", False)):
        monkeypatch.setattr(_autograd, "_ENABLED", [])
        if value is None:
            monkeypatch.delenv("BF_TORCH_DEVICE_ROUTE", raising=False)
        else:
            monkeypatch.setenv("BF_TORCH_DEVICE_ROUTE", value)
        assert _autograd.enabled() is want, value
    monkeypatch.setattr(_autograd, "_ENABLED", [])


def test_the_pointer_check_refuses_without_a_gpu_and_says_nothing():
    """NULL and host memory are no device memory on any box; the library's error message stays what it was"""
    from bodyfitting_amd import _lib, native
    lib = _lib.load()
    said = lib.bf_last_error()
    host = np.zeros(4, np.float32)
    assert native.device_pointer_check(0, 0) is False
    assert native.device_pointer_check(0, host.ctypes.data) is False
    assert lib.bf_last_error() == said
