#!/usr/bin/env python3
"""Frame-loop probe behind profiles/lane_hold.md: the bench's headline loop (bench.FrameFeed + stage_inputs + fit(RESET | FETCH |
NOTIME), 48 views, 100 iterations, 16 frame sets) in brackets of K steps and a sync, as bench.py times them - but with the group
shapes (bf_batch_lane_stats / bf_batch_lane_feed_stats) and a host-clock timeline of one bracket printed, which bench.py cannot show.

  python tools/probe_lane_hold.py shapes [--brackets 11] [--steps 100]   group shapes, per-bracket wall, timeline of the last bracket
  python tools/probe_lane_hold.py latency [--trips 50]                   sequential stage; fit; get_result round trips
  python tools/probe_lane_hold.py drain [--trips 50]                     bf_batch_sync alone: entered with every lane idle and one result held in a lane
  python tools/probe_lane_hold.py trace-summary DIR [--handover store]   durations by kernel and grid from a rocprofv3 --kernel-trace run; lane cycle
                                                                         and tail by G (store: the tail ends with the joints pass, which hands over)

The BF_* settings are the process's environment (the library reads them once).  One JSON line per mode on stdout."""
import argparse
import collections
import csv
import gc
import glob
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def setup(views):
    import bench
    from bodyfitting_amd import _lib, native as N, synthetic as S
    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    dev = N.DeviceModel(model, gmm, device=0)
    batch = bench.build_batch(dev, model, [0], views)
    feed = bench.FrameFeed(model, 0, 1, views, 16)
    flags = _lib.FIT_FETCH | _lib.FIT_NOTIME | _lib.FIT_RESET
    return batch, feed, flags


def shapes(a):
    batch, feed, flags = setup(a.views)
    for _ in range(16 + a.warmup):                       # every frame set through the staging path once, then the warm-up steps
        batch.stage_inputs(*feed.next()); batch.fit(a.iters, flags=flags)
    batch.sync()
    per_bracket, timeline = [], []
    for k in range(a.brackets):
        gc.collect(); gc.disable()
        batch.sync()
        s0 = batch.lane_stats()
        trace = k == a.brackets - 1
        t0 = time.perf_counter_ns()
        for i in range(a.steps):
            batch.stage_inputs(*feed.next())
            t1 = time.perf_counter_ns() if trace else 0
            batch.fit(a.iters, flags=flags)
            if trace:                                    # (reading the counters costs a call each: the last bracket only, reported apart)
                timeline.append((t1 - t0, time.perf_counter_ns() - t0, batch.lane_stats()["launches"] - s0["launches"]))
        t_fed = time.perf_counter_ns()
        batch.sync()
        t_end = time.perf_counter_ns()
        gc.enable()
        s1 = batch.lane_stats()
        rec = {"wall_us": (t_end - t0) / 1e3, "feed_us": (t_fed - t0) / 1e3, "launches": s1["launches"] - s0["launches"]}
        if not trace:
            per_bracket.append(rec)
    plain = [r["wall_us"] for r in per_bracket]
    # the launches of the traced bracket: at which call each went out, when, and how many calls it carried (one group is open at a time and
    # groups go out in order, so a launch carries every call since the one before it; what the sync sends comes last)
    groups, sent, seen = [], 0, 0
    for i, (_, t_fit_end, n) in enumerate(timeline):
        while seen < n:
            seen += 1
            groups.append({"at_call": i, "t_us": round(t_fit_end / 1e3, 1), "G": i + 1 - sent})
            sent = i + 1
    if sent < a.steps:
        groups.append({"at_call": "sync", "G": a.steps - sent})
    fit_us = [(e - s) / 1e3 for s, e, _ in timeline]
    out = {"mode": "shapes", "env": {k: v for k, v in os.environ.items() if k.startswith("BF_FIT_")}, "steps": a.steps,
           "bracket_wall_us": {"median": statistics.median(plain), "min": min(plain), "max": max(plain), "all": [round(x) for x in plain]},
           "frames_per_s_median": a.steps / statistics.median(plain) * 1e6,
           "feed_us_median": statistics.median(r["feed_us"] for r in per_bracket),
           "sync_wait_us": {"median": statistics.median(r["wall_us"] - r["feed_us"] for r in per_bracket),
                            "min": min(r["wall_us"] - r["feed_us"] for r in per_bracket), "max": max(r["wall_us"] - r["feed_us"] for r in per_bracket)},
           "launches_per_bracket": [r["launches"] for r in per_bracket],
           "lane_stats": batch.lane_stats(), "feed_stats": batch.lane_feed_stats(),
           "traced_bracket": {"groups": groups, "fit_call_us_first8": [round(x, 1) for x in fit_us[:8]],
                              "fit_call_us_median": round(statistics.median(fit_us), 2),
                              "call_start_us": [round(s / 1e3, 1) for s, _, _ in timeline[::10]]}}
    print(json.dumps(out))


def latency(a):
    batch, feed, flags = setup(a.views)
    for _ in range(20):
        batch.stage_inputs(*feed.next()); batch.fit(a.iters, flags=flags); batch.get_result()
    trips = []
    for _ in range(a.trips):
        t0 = time.perf_counter_ns()
        batch.stage_inputs(*feed.next()); batch.fit(a.iters, flags=flags); batch.get_result()
        trips.append((time.perf_counter_ns() - t0) / 1e3)
    print(json.dumps({"mode": "latency", "env": {k: v for k, v in os.environ.items() if k.startswith("BF_FIT_")}, "trips": a.trips,
                      "round_trip_us": {"median": statistics.median(trips), "min": min(trips), "max": max(trips)}, "lane_stats": batch.lane_stats()}))


def drain(a):
    """the drain alone: a call that goes out at once (a lone call after a pause finds its lane idle), a pause in which its lane finishes,
    then bf_batch_sync on the host clock - nothing to wait for but what the drain itself issues to hand the result back to the batch"""
    batch, feed, flags = setup(a.views)
    for _ in range(20):
        batch.stage_inputs(*feed.next()); batch.fit(a.iters, flags=flags); batch.sync()
    us = []
    for _ in range(a.trips):
        batch.stage_inputs(*feed.next()); batch.fit(a.iters, flags=flags)
        time.sleep(0.003)
        t0 = time.perf_counter_ns()
        batch.sync()
        us.append((time.perf_counter_ns() - t0) / 1e3)
    st = batch.lane_stats()
    assert st["launches"] == st["calls"] == 20 + a.trips, st           # (every call went out alone, before its pause)
    print(json.dumps({"mode": "drain", "env": {k: v for k, v in os.environ.items() if k.startswith("BF_")}, "trips": a.trips,
                      "sync_us": {"median": statistics.median(us), "min": min(us), "max": max(us)}, "lane_stats": st}))


def trace_summary(a):
    f = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True))
    assert f, "no kernel_trace.csv under " + a.dir
    rows = list(csv.DictReader(open(f[0])))
    by = collections.defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        wg = [max(int(r.get(f"Workgroup_Size_{d}", 1) or 1), 1) for d in "XYZ"]
        grid = tuple(int(r[f"Grid_Size_{d}"]) // w for d, w in zip("XYZ", wg))
        by[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (name, grid), d in sorted(by.items()):
        if "mesh" in name or "fit" in name or "joints" in name or "publish" in name:
            out.append({"kernel": name[:60], "grid": grid, "n": len(d), "median_us": round(statistics.median(d), 2), "min_us": round(min(d), 2), "max_us": round(max(d), 2)})
    # lane cycles: a fit dispatch of G workgroups, the mesh and joints dispatches behind it on the same queue, and - where the copies were
    # traced too - the first device-to-host copy that starts after the joints pass
    copies = []
    for c in sorted(glob.glob(os.path.join(a.dir, "**", "*memory_copy_trace.csv"), recursive=True))[:1]:
        for r in csv.DictReader(open(c)):
            if "DEVICE_TO_HOST" in r.get("Direction", "").upper() or "D2H" in r.get("Direction", "").upper():
                copies.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    copies.sort()
    qkey = "Queue_Id" if rows and "Queue_Id" in rows[0] else None
    cycles, tails = collections.defaultdict(list), collections.defaultdict(list)
    if qkey:
        perq = collections.defaultdict(list)
        for r in rows:
            perq[r[qkey]].append(r)
        for q, rs in perq.items():
            rs.sort(key=lambda r: int(r["Start_Timestamp"]))
            for i, r in enumerate(rs):
                if "fit_kernel<" not in r["Kernel_Name"]:
                    continue
                G = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)
                nxt = [x for x in rs[i + 1:i + 4] if "joints" in x["Kernel_Name"]]
                if not nxt:
                    continue
                j_end = int(nxt[0]["End_Timestamp"])
                end = next((e for s, e in copies if s >= j_end), None) if G * 82680 * 4 >= 512 * 1024 and a.handover == "copy" else None
                if end is None and a.handover == "store":
                    end = j_end
                if end is None:
                    pub = [x for x in rs[i + 1:i + 5] if "publish_kernel" in x["Kernel_Name"] and int(x["Start_Timestamp"]) >= j_end]
                    end = int(pub[0]["End_Timestamp"]) if pub else j_end
                cycles[G].append((end - int(r["Start_Timestamp"])) / 1e3)
                tails[G].append((end - int(r["End_Timestamp"])) / 1e3)
    print(json.dumps({"mode": "trace-summary", "file": f[0], "kernels": out,
                      "lane_cycle_us_by_G": {G: {"n": len(d), "median": round(statistics.median(d), 1), "min": round(min(d), 1), "max": round(max(d), 1)}
                                             for G, d in sorted(cycles.items())},
                      "tail_us_by_G": {G: {"n": len(d), "median": round(statistics.median(d), 1), "min": round(min(d), 1), "max": round(max(d), 1)}
                                       for G, d in sorted(tails.items())},
                      "d2h_copies": len(copies)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("shapes", "latency", "drain", "trace-summary"))
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--brackets", type=int, default=11)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--trips", type=int, default=50)
    ap.add_argument("--handover", choices=("copy", "store"), default="copy")
    a = ap.parse_args()
    {"shapes": shapes, "latency": latency, "drain": drain, "trace-summary": trace_summary}[a.mode](a)
