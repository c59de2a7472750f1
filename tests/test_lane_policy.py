"""The decisions that shape a fit-lane bracket (bodyfitting_amd/csrc/lane_policy.h) on the host alone: a stand-alone program
(tests/lane_policy_main.cpp) built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.  It
prints what the three functions return for every case; the expected values are worked out here, from the rules themselves:

sizing       d = min(lanes wanted, max(n_cus, 1) // F); n_lanes = d if d > 1 and not zerocopy else 1;
             W = min(width wanted, max(1, max(n_cus, 1) // (n_lanes * F)))
close first  n_iters differs, or the hyper-parameter bytes differ, or (W > 1 and the feeding kind differs)
after join   full (n_open >= W): launch; else BF_FIT_LANE_FILL: hold; else hold while W > 1 and the feeder is fast (there was a call
             before, less than H ago) and the group is young (its first call less than H ago) - both strictly; else launch if idle"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = (1, 2, 7, 8, 9, 32, 33, 64, 128, 129, 256, 300)
WANTED_LANES = (1, 4, 32)
WANTED_WIDTH = (1, 32, 64)
WIDTHS = (1, 2, 32)
HOLDS_US = (0, 100)


def gaps_ns(H):
    """0, H - 1 us, H, H + 1 us, and a nanosecond either side of H"""
    g = {0, H * 1000, (H + 1) * 1000, H * 1000 + 1}
    if H > 0:
        g |= {(H - 1) * 1000, H * 1000 - 1}
    return sorted(g)


def want_sizing(n_cus, F, lanes, width, zerocopy):
    cus = max(n_cus, 1)
    d = min(lanes, cus // F)
    n_lanes = d if (not zerocopy and d > 1) else 1
    return n_lanes, min(width, max(1, cus // (n_lanes * F)))


def want_after_join(W, n_open, fill, H, called, gap_prev, gap_first):
    if n_open >= W:
        return "launch"
    if fill:
        return "hold"
    fast_feed = called and gap_prev < H * 1000
    return "hold" if (W > 1 and fast_feed and gap_first < H * 1000) else "if_idle"


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lane_policy") / "lane_policy")
    # the sanitizers' runtimes linked into the program (clang does so by default): it runs as it is, whatever else the process loads
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    "-Wall", "-Werror", "-I", os.path.join(REPO, "bodyfitting_amd", "csrc"), os.path.join(REPO, "tests", "lane_policy_main.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def got(report):
    """{(kind, inputs...): result words} of every line the program printed"""
    out = {}
    for ln in report.stdout.splitlines():
        left, right = ln.split(" -> ")
        kind, *args = left.split()
        key = (kind,) + tuple(int(a) for a in args)
        assert out.get(key, right.split()) == right.split(), ln          # (the same case twice: the same answer)
        out[key] = right.split()
    return out


def test_program_ran_clean(report, got):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-4000:]
    assert report.stderr.strip() == "", report.stderr[-4000:]
    n_size = 2 * len(FRAMES) * len(WANTED_LANES) * len(WANTED_WIDTH) * 2
    n_join = sum(len({1, max(W - 1, 1), W}) * 2 * 2 * len(gaps_ns(H)) ** 2 for W in WIDTHS for H in HOLDS_US)
    assert len([k for k in got if k[0] == "size"]) == n_size
    assert len([k for k in got if k[0] == "join"]) == n_join
    assert len([k for k in got if k[0] == "close"]) == len(WIDTHS) * 8 and len([k for k in got if k[0] == "feed"]) == len(WIDTHS) * 4


@pytest.mark.parametrize("zerocopy", [0, 1])
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("n_cus", [256, 0])
def test_sizing(got, n_cus, F, zerocopy):
    for lanes in WANTED_LANES:
        for width in WANTED_WIDTH:
            n_lanes, W = want_sizing(n_cus, F, lanes, width, zerocopy)
            assert got[("size", n_cus, F, lanes, width, zerocopy)] == [str(n_lanes), str(W)], (lanes, width)
            # what the formula is for: the lanes' full groups never ask for more than a frame per CU, unless one call alone does
            assert 1 <= n_lanes <= lanes and 1 <= W <= width
            assert n_lanes * W * F <= max(n_cus, 1) or (n_lanes == 1 and W == 1)
            assert not (zerocopy and n_lanes > 1)


@pytest.mark.parametrize("W", WIDTHS)
def test_close_before_join(got, W):
    for iters_differ in (0, 1):
        for hyper_differ in (0, 1):
            for feed_differs in (0, 1):
                want = bool(iters_differ or hyper_differ or (W > 1 and feed_differs))
                assert got[("close", W, iters_differ, hyper_differ, feed_differs)] == [str(int(want))], (iters_differ, hyper_differ, feed_differs)
    for open_host in (0, 1):
        for host_fed in (0, 1):
            assert got[("feed", W, open_host, host_fed)] == [str(int(W > 1 and open_host != host_fed))]


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("H", HOLDS_US)
@pytest.mark.parametrize("W", WIDTHS)
def test_after_join(got, W, H, fill):
    seen = set()
    for n_open in sorted({1, max(W - 1, 1), W}):
        for called in (0, 1):          # 0: the first LANE-route call of the batch
            for gap_prev in gaps_ns(H):
                for gap_first in gaps_ns(H):
                    want = want_after_join(W, n_open, fill, H, called, gap_prev, gap_first)
                    assert got[("join", W, n_open, fill, H, called, gap_prev, gap_first)] == [want], (n_open, called, gap_prev, gap_first)
                    seen.add(want)
    # the case list reaches every outcome the rule has for this (W, H, fill)
    assert "launch" in seen
    if W > 1:
        assert ("hold" in seen) == bool(fill or H > 0)
        assert ("if_idle" in seen) == (not fill)
    else:
        assert seen == {"launch"}
