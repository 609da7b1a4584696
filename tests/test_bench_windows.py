"""profiles/tools/bench_windows.measure on the host: a scripted timer in place of the device events."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tools"))
import bench_windows as bw  # noqa: E402


class FakeTimer:
    """timer(call, calls): logs (variant name or None, calls), runs the call once, returns the next scripted time."""

    def __init__(self, variants, seconds):
        self.names = {call: name for name, call in variants.items()}
        self.seconds = {name: list(ts) for name, ts in seconds.items()}
        self.log = []

    def __call__(self, call, calls):
        name = self.names.get(call)
        self.log.append((name, calls))
        call(0)
        return self.seconds[name].pop(0) if name else 0.0


def _noop(i):
    pass


def _variants(*names):
    return {name: (lambda i: None) for name in names}


@pytest.mark.parametrize("per_call, script, passes, calls", [
    (0.016, [0.016, 0.016], [3, 5], 13),                 # 50 * 0.016 >= 0.2: no 50-call pass; int(12.5) + 1
    (1e-4, [1e-4, 1e-4, 2e-4], [3, 5, 50], 1001),        # the 50-call pass's value is the one used: int(1000.0) + 1
    (1.0, [1.0, 1.0], [3, 5], 3),                        # never fewer than 3 calls
])
def test_window_sizing(per_call, script, passes, calls):
    variants = _variants("a")
    timer = FakeTimer(variants, {"a": script + [per_call]})
    results, failed = bw.measure(variants, 0.2, 1, timer)
    assert timer.log == [("a", n) for n in passes] + [("a", calls)]
    assert failed == {} and list(results) == ["a"]


def test_order_and_statistics():
    variants = _variants("a", "b")
    timer = FakeTimer(variants, {"a": [0.016, 0.016, 1.0, 3.0, 2.0], "b": [1e-4, 1e-4, 2e-4, 5.0, 5.0, 5.0]})
    results, failed = bw.measure(variants, 0.2, 3, timer)
    assert timer.log == [("a", 3), ("a", 5), ("b", 3), ("b", 5), ("b", 50)] + [("a", 13), ("b", 1001)] * 3
    assert failed == {}
    assert results["a"].median == 2.0 and results["a"].spread == 1.0 and results["a"].times == [1.0, 3.0, 2.0]
    assert results["b"].median == 5.0 and results["b"].spread == 0.0 and results["b"].times == [5.0, 5.0, 5.0]


def test_failing_variant_is_dropped_and_the_device_probed():
    def boom(i):
        raise RuntimeError("boom\nmore")
    variants = {"a": _noop, "x": boom, "b": lambda i: None}
    timer = FakeTimer(variants, {"a": [1.0, 1.0, 1.0, 1.0], "b": [1.0, 1.0, 2.0, 2.0], "x": []})
    results, failed = bw.measure(variants, 0.2, 2, timer)
    assert failed == {"x": "boom"}
    assert timer.log == [("a", 3), ("a", 5), ("x", 3), (None, 1), ("b", 3), ("b", 5)] + [("a", 3), ("b", 3)] * 2
    assert sorted(results) == ["a", "b"]
    assert results["a"].times == [1.0, 1.0] and results["b"].times == [2.0, 2.0]


def test_failure_message_is_cut_to_120_characters():
    def long(i):
        raise RuntimeError("m" * 300)
    variants = {"x": long}
    _, failed = bw.measure(variants, 0.2, 1, FakeTimer(variants, {"x": []}))
    assert failed == {"x": "m" * 120}


def test_other_exceptions_propagate():
    def bad(i):
        raise ValueError("not a runtime error")
    variants = {"a": _noop, "x": bad}
    timer = FakeTimer(variants, {"a": [1.0, 1.0], "x": []})
    with pytest.raises(ValueError):
        bw.measure(variants, 0.2, 1, timer)
    assert timer.log == [("a", 3), ("a", 5), ("x", 3)]


def test_rotation_sets():
    assert bw.rotation_sets(bw.CACHE_BYTES) == 2
    assert bw.rotation_sets(4 * bw.CACHE_BYTES) == 2
    assert bw.rotation_sets(bw.CACHE_BYTES // 2) == 2
    assert bw.rotation_sets(bw.CACHE_BYTES // 3) == 4             # 178956970 B: three sets fall 2 B short
    assert bw.rotation_sets(1 << 20) == 512
    assert bw.rotation_sets((1 << 20) + 1) == 512                 # ceil(511.9995...)
    assert bw.rotation_sets((1 << 20) - 1) == 513


def test_small_helpers():
    import torch
    assert bw.dtype_name(torch.float32) == "fp32" and bw.dtype_name(torch.float64) == "fp64"
    bw.checked(0, "call")
    with pytest.raises(RuntimeError, match="call returned status 3"):
        bw.checked(3, "call")
    a = bw.parser(0.15).parse_args([])
    assert (a.window, a.reps, a.out) == (0.15, 5, None)


def test_finish_writes_what_it_returns(tmp_path):
    out = tmp_path / "table.md"
    text = bw.finish(["| a |", "|---|"], 0.2, 3, str(out))
    assert text == "windows of >= 0.20 s, 3 alternated windows per variant\n\n| a |\n|---|\n"
    assert out.read_text() == text
    assert bw.finish(["x"], 0.2, 3, None, head="own header") == "own header\n\nx\n"
