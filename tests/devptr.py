"""One C-ABI call run through every pointer route -- host arrays, device arrays, and the two mixtures -- and compared
(tests/test_gpu_device_pointers.py on the device, tests/test_devptr_host.py for the checker itself on CPU tensors).

The caller describes a call once:

    fn(p) -> status      ``p`` maps every array's name to its raw address (an int); the callable forms the argument list
    inputs               name -> NumPy array
    outputs              name -> ``Out(shape, dtype)``  (``init``: the bytes the output holds before the call -- an in-place call)
    host_only            names that are NumPy arrays on every route (what the library dereferences on the host)
    odd                  inputs that the ``device_odd`` route places at an odd element offset (8-byte aligned only)

Route ``host`` is the expectation.  After every other route: the status is the host route's, every output has the host
route's bits (compared as bytes: NaN payloads count), the 64 sentinel doubles on either side of every output are intact,
and every input still has the bits it was given.  Every failure names the entry, the route and the array.
"""
import collections
import ctypes

import numpy as np

GUARD = 64 * 8                                   # bytes on either side of every output: 64 doubles
SENTINEL = np.array([0x7FF8DEADBEEF1234], dtype=np.uint64).view(np.uint8)      # as a double: a NaN with a payload
ROUTES = ("host", "device", "in_device_out_host", "in_host_out_device", "device_odd")

Out = collections.namedtuple("Out", "shape dtype init")
Out.__new__.__defaults__ = (None,)


class Mismatch(AssertionError):
    pass


def _sentinel_bytes(nbytes, phase=0):
    """``nbytes`` of the repeated sentinel, starting ``phase`` bytes into it"""
    reps = (nbytes + phase) // 8 + 2
    return np.tile(SENTINEL, reps)[phase:phase + nbytes].copy()


def _nbytes(shape, dtype):
    return int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize


class _Buf(object):
    """``payload`` bytes with ``lead`` / ``trail`` sentinel bytes around them, in host memory (``device is None``) or in a flat
    uint8 tensor on ``device``"""

    def __init__(self, payload, lead, trail, device):
        self.lead, self.n = lead, len(payload)
        flat = np.concatenate([_sentinel_bytes(lead), payload, _sentinel_bytes(trail, (lead + len(payload)) % 8)])
        if device is None:
            self.t, self.a = None, flat
            base = flat.ctypes.data
        else:
            import torch
            self.t = torch.from_numpy(flat).to(device)
            self.a = None
            base = self.t.data_ptr()
        self.initial = flat.copy()
        self.addr = base + lead

    def bytes(self):
        """the whole buffer now, guards included, as host bytes"""
        return self.a.copy() if self.t is None else self.t.cpu().numpy()

    def pristine_copy(self):
        return None if self.t is None else self.t.clone()


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return int(d[0]) if len(d) else -1


def as_array(address, shape, dtype):
    """a NumPy view of host memory at ``address`` (for stand-in entry points written in NumPy)"""
    n = _nbytes(shape, dtype)
    raw = (ctypes.c_uint8 * n).from_address(address)
    return np.frombuffer(raw, dtype=dtype).reshape(shape)


def run_route(entry, route, fn, inputs, outputs, host_only=(), odd=(), device="cuda", prepare=None, sync=None):
    """One route of one call: ``(status, {name: output array})`` after the guard-band and the untouched-input checks."""
    if sync is None:
        def sync():
            if str(device).startswith("cuda"):
                import torch
                torch.cuda.synchronize()
    in_dev = route in ("device", "in_device_out_host", "device_odd")
    out_dev = route in ("device", "in_host_out_device", "device_odd")
    if prepare is not None:
        prepare()
    bufs, pristine, p = {}, {}, {}
    for name, a in inputs.items():
        a = np.ascontiguousarray(a)
        where = device if (in_dev and name not in host_only) else None
        lead = a.dtype.itemsize if (route == "device_odd" and name in odd and where is not None) else 0
        b = _Buf(a.reshape(-1).view(np.uint8), lead, 0, where)
        bufs[name], pristine[name] = b, b.pristine_copy()
        p[name] = b.addr
    for name, o in outputs.items():
        n = _nbytes(o.shape, o.dtype)
        payload = _sentinel_bytes(n) if o.init is None else np.ascontiguousarray(o.init).reshape(-1).view(np.uint8)
        assert len(payload) == n, (entry, name)
        where = device if (out_dev and name not in host_only) else None
        bufs[name] = _Buf(payload, GUARD, GUARD, where)
        p[name] = bufs[name].addr
    sync()                                       # the caller guarantees that its inputs are ready
    rc = fn(p)
    sync()
    got = {}
    for name, o in outputs.items():
        b = bufs[name]
        now = b.bytes()
        for side, sl in (("front", slice(0, b.lead)), ("back", slice(b.lead + b.n, None))):
            at = _first_diff(now[sl], b.initial[sl])
            if at >= 0:
                raise Mismatch("%s [%s] output %s: the %s guard band was written at byte %d of %d"
                               % (entry, route, name, side, at, len(now[sl])))
        got[name] = now[b.lead:b.lead + b.n].view(o.dtype).reshape(o.shape).copy()
    for name in inputs:
        b = bufs[name]
        if b.t is not None:
            import torch
            same = bool(torch.equal(b.t, pristine[name]))
            at = -1 if same else _first_diff(b.bytes(), b.initial)
        else:
            at = _first_diff(b.a, b.initial)
        if at >= 0:
            raise Mismatch("%s [%s] input %s: changed by the call at byte %d" % (entry, route, name, at - b.lead))
    return rc, got


def compare(entry, route, expect, got, whose="the host route's"):
    """status and outputs of ``route`` against the host route's (or ``whose``), bit for bit"""
    (rc0, out0), (rc, out) = expect, got
    if rc != rc0:
        raise Mismatch("%s [%s]: status %r, %s is %r" % (entry, route, rc, whose, rc0))
    for name, ref in out0.items():
        a, b = ref.reshape(-1).view(np.uint8), out[name].reshape(-1).view(np.uint8)
        at = _first_diff(a, b)
        if at >= 0:
            k = at // ref.dtype.itemsize
            raise Mismatch("%s [%s] output %s: element %d of %d is %r, %s is %r (first differing byte %d)"
                           % (entry, route, name, k, ref.size, out[name].reshape(-1)[k].item(), whose, ref.reshape(-1)[k].item(), at))


def check_routes(entry, fn, inputs, outputs, host_only=(), odd=(), device="cuda", prepare=None, routes=ROUTES, sync=None):
    """The call on every route; returns ``{route: (status, outputs)}`` for further checks against a reference."""
    res = {}
    for route in routes:
        if route == "device_odd" and not any(name in inputs and name not in host_only for name in odd):
            continue
        res[route] = run_route(entry, route, fn, inputs, outputs, host_only, odd, device, prepare, sync)
        if route != "host":
            compare(entry, route, res["host"], res[route])
    return res
