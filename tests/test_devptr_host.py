"""The checker of tests/devptr.py can fail: CPU tensors stand in for device memory and NumPy functions for the entry points,
each wrong in one way.  Needs neither a GPU nor the native library."""
import numpy as np
import pytest

import torch  # noqa: F401  (the checker makes its "device" arrays with it)

import devptr
from devptr import Out

N1 = 37          # odd: the byte offsets of the guard bands are exercised off the 16-byte grid too


def _inputs():
    rng = np.random.RandomState(5)
    return {"x": rng.randn(N1), "w": rng.randn(N1)}


def _outputs():
    return {"out": Out((N1,), np.float64), "rank": Out((1,), np.int64)}


def _correct(p):
    x, w = devptr.as_array(p["x"], (N1,), np.float64), devptr.as_array(p["w"], (N1,), np.float64)
    out = devptr.as_array(p["out"], (N1,), np.float64)
    out[:] = x * w
    out[3] = np.nan
    devptr.as_array(p["rank"], (1,), np.int64)[0] = 7
    return 0


def _run(fn, **kw):
    return devptr.check_routes("fake", fn, _inputs(), _outputs(), odd=("x",), device="cpu", **kw)


def _on_device_routes(wrong):
    """``wrong`` everywhere but on the host route (whose pointers are the first the checker hands out): the call counter tells"""
    calls = {"n": 0}

    def fn(p):
        calls["n"] += 1
        rc = _correct(p)
        return wrong(p, rc) if calls["n"] > 1 else rc
    return fn


def test_a_correct_entry_passes_every_route():
    res = _run(_correct)
    assert set(res) == set(devptr.ROUTES)
    for route, (rc, out) in res.items():
        assert rc == 0 and out["rank"][0] == 7 and np.isnan(out["out"][3])
        x = _inputs()
        assert np.array_equal(np.delete(out["out"], 3), np.delete(x["x"] * x["w"], 3))


def test_the_odd_route_is_eight_byte_aligned_only():
    seen = []

    def fn(p):
        seen.append(p["x"] % 16)
        return _correct(p)
    _run(fn, routes=("host", "device_odd"))
    assert seen[-1] == 8 and seen[0] in (0, 8)


def test_odd_route_is_left_out_without_odd_inputs():
    res = devptr.check_routes("fake", _correct, _inputs(), _outputs(), device="cpu")
    assert "device_odd" not in res and len(res) == 4


def test_one_element_past_the_output_is_caught():
    def wrong(p, rc):
        devptr.as_array(p["out"], (N1 + 1,), np.float64)[N1] = 0.0
        return rc
    with pytest.raises(devptr.Mismatch, match=r"fake \[device\] output out: the back guard band"):
        _run(_on_device_routes(wrong))


def test_one_element_in_front_of_the_output_is_caught():
    def wrong(p, rc):
        devptr.as_array(p["out"] - 8, (1,), np.float64)[0] = 0.0
        return rc
    with pytest.raises(devptr.Mismatch, match=r"fake \[device\] output out: the front guard band"):
        _run(_on_device_routes(wrong))


def test_the_far_end_of_the_guard_band_is_watched_too():
    def wrong(p, rc):
        devptr.as_array(p["out"] + 8 * (N1 + 63), (1,), np.float64)[0] = 1.0
        return rc
    with pytest.raises(devptr.Mismatch, match="back guard band"):
        _run(_on_device_routes(wrong))


def test_a_changed_input_is_caught():
    def wrong(p, rc):
        devptr.as_array(p["w"], (N1,), np.float64)[N1 - 1] *= -1.0       # one sign bit
        return rc
    with pytest.raises(devptr.Mismatch, match=r"fake \[device\] input w: changed by the call at byte %d" % (8 * (N1 - 1) + 7)):
        _run(_on_device_routes(wrong))


def test_a_changed_host_input_is_caught_on_the_mixed_route():
    def wrong(p, rc):
        devptr.as_array(p["x"], (N1,), np.float64)[0] = 0.0
        return rc
    with pytest.raises(devptr.Mismatch, match=r"fake \[in_host_out_device\] input x"):
        _run(_on_device_routes(wrong), routes=("host", "in_host_out_device"))


def test_one_differing_bit_is_caught():
    def wrong(p, rc):
        bits = devptr.as_array(p["out"], (N1,), np.uint64)
        bits[11] ^= np.uint64(1)
        return rc
    with pytest.raises(devptr.Mismatch, match=r"fake \[device\] output out: element 11 of %d" % N1):
        _run(_on_device_routes(wrong))


def test_a_nan_with_another_payload_is_caught():
    def wrong(p, rc):
        bits = devptr.as_array(p["out"], (N1,), np.uint64)
        bits[3] = np.uint64(0x7FF8000000000001)
        return rc
    res = _run(_correct)
    assert np.isnan(res["host"][1]["out"][3])            # a value comparison would see NaN on both sides
    with pytest.raises(devptr.Mismatch, match=r"output out: element 3 "):
        _run(_on_device_routes(wrong))


def test_an_integer_output_is_compared():
    def wrong(p, rc):
        devptr.as_array(p["rank"], (1,), np.int64)[0] = 6
        return rc
    with pytest.raises(devptr.Mismatch, match=r"output rank: element 0 of 1 is 6, the host route's is 7"):
        _run(_on_device_routes(wrong))


def test_another_status_is_caught():
    with pytest.raises(devptr.Mismatch, match=r"fake \[device\]: status 3, the host route's is 0"):
        _run(_on_device_routes(lambda p, rc: 3))


def test_an_output_left_unwritten_is_caught():
    def wrong(p, rc):
        devptr.as_array(p["out"], (N1,), np.uint64)[N1 - 1] = devptr.SENTINEL.view(np.uint64)[0]
        return rc
    with pytest.raises(devptr.Mismatch, match=r"output out: element %d " % (N1 - 1)):
        _run(_on_device_routes(wrong))


def test_host_only_names_stay_numpy_and_prepare_runs_before_every_route():
    count = {"prepare": 0}
    inputs = dict(_inputs(), which=np.ones(3, dtype=np.uint32))
    host_addresses = []

    def fn(p):
        host_addresses.append((p["which"], p["rank"]))
        assert np.array_equal(devptr.as_array(p["which"], (3,), np.uint32), [1, 1, 1])
        return _correct(p)

    def prepare():
        count["prepare"] += 1
    res = devptr.check_routes("fake", fn, inputs, _outputs(), host_only=("which", "rank"), odd=("x", "which"), device="cpu",
                              prepare=prepare)
    assert count["prepare"] == len(res) == 5
    assert all(a % 4 == 0 for a, _ in host_addresses)       # (never moved to the odd offset)


def test_an_in_place_output_starts_from_its_initial_bytes():
    b = np.arange(12.0).reshape(4, 3)

    def fn(p):
        io = devptr.as_array(p["out"], (4, 3), np.float64)
        io *= 2.0
        return 0
    res = devptr.check_routes("fake", fn, {}, {"out": Out((4, 3), np.float64, b)}, device="cpu")
    for rc, out in res.values():
        assert np.array_equal(out["out"], 2.0 * b)
    assert np.array_equal(b, np.arange(12.0).reshape(4, 3))
