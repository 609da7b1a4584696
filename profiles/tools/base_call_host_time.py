"""Host cost of one call of _lib.tail_log_prob and _lib.gmm_log_prob at B = 1, D = 8, fp32, no_grad: the median wall time
of 2000 calls after 200 warm-up calls, (a) the call alone (the enqueue: what the dispatch is part of) and (b) the call
and a device synchronise.  The library is the in-tree one, or VCNF_LIB (profiles/stream_dispatch.md section 5 runs it
as parent / new / parent / new, one process each).  Usage: base_call_host_time.py LABEL OUT.json"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import vcnf_amd as nf
from vcnf_amd import _lib

label, out = sys.argv[1], sys.argv[2]
assert torch.cuda.is_available()
nf.lib()
torch.manual_seed(0)
D, M = 8, 4
dev = "cuda:0"
z = torch.randn(1, D, device=dev)
loc, ls = torch.randn(D, device=dev), 0.1 * torch.randn(D, device=dev)
shape, cst = torch.full((D,), 4.0, device=dev), torch.zeros(D, device=dev)
gloc, gls, glw = torch.randn(M, D, device=dev), 0.1 * torch.randn(M, D, device=dev), torch.log_softmax(torch.randn(M, device=dev), 0)
calls = {
    "tail_log_prob": lambda: _lib.tail_log_prob(z, loc, ls, shape, cst, _lib.TAIL_STUDENT_T),
    "gmm_log_prob": lambda: _lib.gmm_log_prob(z, gloc, gls, glw),
}


def median_us(fn, sync):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(2000):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return 1e6 * statistics.median(times)


res = {"label": label, "lib": _lib.lib_path()}
with torch.no_grad():
    for name, fn in calls.items():
        assert torch.isfinite(fn()).all()
        res[name + "_enqueue_us"] = round(median_us(fn, False), 3)
        res[name + "_synced_us"] = round(median_us(fn, True), 3)
print(json.dumps(res), flush=True)
with open(out, "w") as f:
    json.dump(res, f)
