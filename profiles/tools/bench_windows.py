"""The timing protocol of the profiles/tools/*_bench.py drivers, stated once.

A window is `calls` back-to-back calls between two device events; time per call = window / calls, launches and Python
included.  Per variant, in the order given: a warm-up window of 3 calls, a calibration window of 5 and, where 50 such
calls would not fill the window, one of 50 (a 5-call window of a launch-bound call is mostly the events' own cost); the
timed windows then hold enough calls to last at least --window seconds, and never fewer than 3.  The variants of one
group are alternated for --reps windows each, so drift of the machine lands on all of them alike; a table row gives the
median of a variant's windows and their spread (max - min) / median.

A variant whose warm-up or calibration raises a RuntimeError (out of memory, a library's allocation failure, a status
the kernel returns) is dropped and gets a `failed: <message>` row; the others are measured.  Before anything else is
launched one empty window is recorded and synchronised outside any handler, so an error that has left the device unusable
surfaces there and ends the tool.

The rotating tools walk successive calls over enough buffer sets to exceed CACHE_BYTES, twice the 256 MiB Infinity
Cache, so their rows come from HBM.  Importing this module puts the repository root and tests/ (the plain-torch
restatements) on sys.path; it needs no GPU.
"""
import argparse
import collections
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8e12                   # bytes / s, as specified; a float4 copy measures 6.29e12 on this part
CACHE_BYTES = 512 << 20           # rotate over at least this much input: twice the Infinity Cache
HEAD = "windows of >= %.2f s, %d alternated windows per variant"

Result = collections.namedtuple("Result", "median spread times")      # seconds per call, (max - min) / median, every window


def rotation_sets(bytes_per_set):
    return max(2, -(-CACHE_BYTES // bytes_per_set))


def dtype_name(dtype):
    return "fp64" if dtype == torch.float64 else "fp32"


def checked(status, what):
    if status != 0:
        raise RuntimeError("%s returned status %d" % (what, status))


def window_seconds(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        call(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls          # seconds per call


def measure(variants, window, reps, timer=window_seconds):
    """({name: Result}, {name: message}) for variants = {name: call(i)}; a name is in exactly one of the two."""
    calls, failed = {}, {}
    for name, call in variants.items():
        try:                                           # warm-up, then size the window
            timer(call, 3)
            t = timer(call, 5)
            if 50 * t < window:
                t = timer(call, 50)
            calls[name] = max(3, int(window / t) + 1)
        except RuntimeError as e:                      # a variant that cannot run at this shape
            failed[name] = (str(e).splitlines() or [""])[0][:120]
        if name in failed:
            if torch.cuda.is_initialized():
                torch.cuda.empty_cache()
            timer(lambda i: None, 1)                   # a device the failure broke raises here, uncaught
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name in calls:
            times[name].append(timer(variants[name], calls[name]))
    results = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        results[name] = Result(med, (max(ts) - min(ts)) / med, ts)
    return results, failed


def parser(window):
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=window, help="least seconds per timed window")
    ap.add_argument("--reps", type=int, default=5, help="alternated windows per variant")
    ap.add_argument("--out", default=None, help="file the table is written to")
    return ap


def finish(lines, window, reps, out, head=None):
    text = "%s\n\n%s\n" % (head or HEAD % (window, reps), "\n".join(lines))
    if out:
        with open(out, "w") as f:
            f.write(text)
    return text
