"""The two-level dense Cholesky driver executes a launch list (george_amd/csrc/gh_chol_plan.h); gh_debug_chol_plan returns that
list without a device.  A wrong wait in such a driver does not fail on the GPU, it flips low bits once in a while -- so the list
is checked here, on the CPU: replayed in NumPy in several legal orders, its conflicting ops ordered through stream order and
events, every block column receiving every earlier panel's k-range exactly once and ascending, every size a multiple of what
the GEMM kernel needs."""
import ctypes as C

import numpy as np
import pytest

PANEL, L, T, F, JOIN = 0, 1, 2, 3, 4
MAIN, CHAIN = 0, 1
COLS = 12
# hide: the group rule's margin "chain of the next group <= hide x far update beside it" (times in ms, calibrated at N >= 24576).
# The default (0) leaves a matrix this small in single panels, i.e. the one-level schedule; a huge value lets every group reach
# the maximum; the values between cut groups back somewhere along the matrix.
CASES = [
    # (Np, nb, bound, gmax, hide)
    (2048, 256, 0, 2, 1e12),
    (2560, 256, 0, 4, 1e12),            # 10 panels
    (2816, 256, 0, 8, 1e12),            # 11 panels (odd)
    (3072 + 128, 512, 1024, 2, 1e12),   # 1024-wide panels, then 512, ragged last panel
    (4096 + 384, 512, 1536, 4, 1e12),
    (6144, 512, 2048, 8, 1e12),
    (6144, 1024, 0, 4, 1e12),
    (5120 + 256, 256, 2560, 4, 300.0),
    (5120 + 256, 256, 2560, 8, 3000.0),
    (4608, 256, 1024, 8, 30000.0),
    (3328, 256, 0, 4, 0.0),             # the default margin: single panels
    (3328, 256, 0, 1, 0.0),             # gmax = 1: the one-level list
]


def get_plan(np_, nb, bound, gmax, hide):
    from george_amd import _native as N
    ns, no, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    N.check(N.lib.gh_debug_chol_plan(np_, nb, bound, gmax, hide, None, 0, C.byref(ns), None, 0, C.byref(no), C.byref(ne)))
    pc = (C.c_int64 * ns.value)()
    ops = (C.c_int64 * (no.value * COLS))()
    N.check(N.lib.gh_debug_chol_plan(np_, nb, bound, gmax, hide, pc, ns.value, C.byref(ns), ops, no.value, C.byref(no), C.byref(ne)))
    ops = np.array(list(ops), dtype=np.int64).reshape(no.value, COLS)
    keys = ("kind", "stream", "r0", "r1", "c0", "c1", "k0", "k1", "wait0", "wait1", "record", "lower")
    return list(pc), [dict(zip(keys, (int(v) for v in row))) for row in ops], ne.value


def preds(ops):
    """per op: the ops that must be complete before it may run (stream predecessor + the recorders of the events it waits for);
    asserts what the executor relies on: an event is recorded by one op, and that op is issued BEFORE any op waiting for it
    (a hipStreamWaitEvent on an event not yet recorded is no wait at all)"""
    rec = {}
    for i, o in enumerate(ops):
        if o["record"] >= 0:
            assert o["record"] not in rec, "event %d recorded twice" % o["record"]
            rec[o["record"]] = i
    last = {}
    out = []
    for i, o in enumerate(ops):
        p = set()
        if o["stream"] in last:
            p.add(last[o["stream"]])
        last[o["stream"]] = i
        for w in (o["wait0"], o["wait1"]):
            if w >= 0:
                assert w in rec and rec[w] < i, "op %d waits for event %d, which no earlier op records" % (i, w)
                p.add(rec[w])
        out.append(p)
    return out


def legal_order(ops, prefer):
    """a schedule in which an op runs once its predecessors are complete; `prefer` picks among the ready ops"""
    P = preds(ops)
    done, order = set(), []
    while len(order) < len(ops):
        ready = [i for i in range(len(ops)) if i not in done and P[i] <= done]
        assert ready, "deadlock"
        i = prefer(ready, ops)
        done.add(i); order.append(i)
    return order


def replay(ops, order, A):
    A = A.copy()
    n = A.shape[0]
    for i in order:
        o = ops[i]
        r0, r1, c0, c1, k0, k1 = (o[k] for k in ("r0", "r1", "c0", "c1", "k0", "k1"))
        if o["kind"] == PANEL:
            d = np.tril(A[c0:c1, c0:c1])
            Lb = np.linalg.cholesky(d + np.tril(d, -1).T)
            A[c0:c1, c0:c1] = Lb
            if c1 < n:
                A[c1:, c0:c1] = np.linalg.solve(Lb, A[c1:, c0:c1].T).T
        elif o["kind"] in (L, T, F):
            upd = A[r0:r1, k0:k1] @ A[c0:c1, k0:k1].T
            if o["lower"]:                                   # tiles on or below the diagonal of the trapezoid only
                tr = (np.arange(r1 - r0) // 128)[:, None]
                tc = (np.arange(c1 - c0) // 128)[None, :]
                upd = np.where(tc <= tr, upd, 0.0)
            A[r0:r1, c0:c1] -= upd
    return np.tril(A)


def spd(n, seed):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0, n / 20.0, n))
    return np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2) + np.diag(0.05 + rng.uniform(0, 0.1, n))


def group_sizes(ops):
    sizes, cur = [], 0
    for o in ops:
        if o["kind"] == PANEL:
            cur += 1
        if o["kind"] in (T, JOIN):
            sizes.append(cur); cur = 0
    return sizes


@pytest.mark.parametrize("case", CASES)
def test_replay_gives_the_cholesky_factor_in_every_legal_order(case):
    np_, nb, bound, gmax, hide = case
    pc, ops, _ = get_plan(*case)
    print("panels", np.diff(pc).tolist(), "groups", group_sizes(ops))
    A = spd(np_, 7)
    ref = np.linalg.cholesky(A)
    rng = np.random.RandomState(3)
    orders = {
        "issue order": list(range(len(ops))),
        "main stream first": legal_order(ops, lambda r, o: min(r, key=lambda i: (o[i]["stream"] != MAIN, i))),
        "chain stream first": legal_order(ops, lambda r, o: min(r, key=lambda i: (o[i]["stream"] != CHAIN, i))),
        "latest ready op first": legal_order(ops, lambda r, o: max(r)),
        "random": legal_order(ops, lambda r, o: r[rng.randint(len(r))]),
    }
    P = preds(ops)
    pos = {i: q for q, i in enumerate(orders["issue order"])}
    assert all(pos[p] < pos[i] for i in range(len(ops)) for p in P[i])          # the issue order is itself legal
    for name, order in orders.items():
        Lf = replay(ops, order, A)
        err = np.abs(Lf - ref).max() / np.abs(ref).max()
        print(name, "max error %.2e" % err)
        # rounding of a blocked against an unblocked factorisation of a matrix with condition number ~1e3: a missing
        # update or a panel read too early is an error of order 1e-3 ... 1
        assert err < 1e-11, (name, err)


def _ancestors(ops):
    P = preds(ops)
    anc = []
    for i in range(len(ops)):                                # list order is topological (asserted in preds)
        a = set()
        for p in P[i]:
            a |= anc[p] | {p}
        anc.append(a)
    return anc


def _rects(o, n):
    """(writes, reads): lists of (row0, row1, col0, col1)"""
    if o["kind"] == JOIN:
        return [], []
    w = [(o["r0"], o["r1"], o["c0"], o["c1"])]
    if o["kind"] == PANEL:
        return w, []
    return w, [(o["r0"], o["r1"], o["k0"], o["k1"]), (o["c0"], o["c1"], o["k0"], o["k1"])]


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1] and a[2] < b[3] and b[2] < a[3]


@pytest.mark.parametrize("case", CASES)
def test_conflicting_ops_are_ordered_through_streams_and_events(case):
    np_, nb, bound, gmax, hide = case
    pc, ops, nev = get_plan(*case)
    anc = _ancestors(ops)
    R = [_rects(o, np_) for o in ops]
    for i in range(len(ops)):
        for j in range(i + 1, len(ops)):
            (wi, ri), (wj, rj) = R[i], R[j]
            conflict = any(_overlap(a, b) for a in wi for b in wj + rj) or any(_overlap(a, b) for a in wj for b in ri)
            if conflict:
                assert i in anc[j], "ops %d %r and %d %r touch the same elements and are not ordered" % (i, ops[i], j, ops[j])
    # the join: the main stream ends behind everything
    assert ops[-1]["kind"] == JOIN and ops[-1]["stream"] == MAIN
    assert anc[len(ops) - 1] == set(range(len(ops) - 1))
    assert sorted(o["record"] for o in ops if o["record"] >= 0) == list(range(nev))


@pytest.mark.parametrize("case", CASES)
def test_every_column_receives_every_earlier_panel_once_and_ascending(case):
    np_, nb, bound, gmax, hide = case
    pc, ops, _ = get_plan(*case)
    assert pc[0] == 0 and pc[-1] == np_ and all(b > a for a, b in zip(pc, pc[1:]))
    anc = _ancestors(ops)
    panels = [i for i, o in enumerate(ops) if o["kind"] == PANEL]
    assert [(ops[i]["c0"], ops[i]["c1"]) for i in panels] == list(zip(pc, pc[1:]))       # every panel once, left to right
    for ip in panels:
        c0, c1 = ops[ip]["c0"], ops[ip]["c1"]
        ups = [i for i, o in enumerate(ops) if o["kind"] in (L, T, F) and o["c0"] < c1 and c0 < o["c1"]]
        at = 0
        for q, i in enumerate(ups):
            o = ops[i]
            assert o["c0"] <= c0 and c1 <= o["c1"] and o["r0"] == o["c0"] and o["r1"] == np_       # whole panel columns, down to the last row
            assert o["k0"] == at and o["k1"] > o["k0"], (c0, [(ops[u]["k0"], ops[u]["k1"]) for u in ups])
            at = o["k1"]
            if q:
                assert ups[q - 1] in anc[i]                  # ... in THAT order on the device, not only in the list
        assert at == c0, (c0, at)                            # everything left of the panel, nothing else
        assert all(i in anc[ip] for i in ups)
        # and whoever reads this panel's columns as an operand runs behind the panel
        for i, o in enumerate(ops):
            if o["kind"] in (L, T, F) and o["k0"] < c1 and c0 < o["k1"]:
                assert ip in anc[i]


@pytest.mark.parametrize("case", CASES)
def test_sizes_suit_the_gemm_kernel_and_groups_respect_the_maximum(case):
    np_, nb, bound, gmax, hide = case
    pc, ops, _ = get_plan(*case)
    rec = {o["record"]: o for o in ops if o["record"] >= 0}
    for o in ops:
        assert all(o[k] % 128 == 0 for k in ("r0", "r1", "c0", "c1", "k0", "k1"))
        if o["kind"] in (L, T, F):
            assert (o["k1"] - o["k0"]) % 32 == 0 and o["k1"] > o["k0"]
            assert o["r1"] - o["r0"] >= o["c1"] - o["c0"] > 0           # a lower trapezoid: M >= N
            assert o["stream"] == (MAIN if o["kind"] == F else CHAIN)
            assert (o["wait1"] < 0) and (o["kind"] != L or o["wait0"] < 0)
            if o["kind"] == F:             # the main stream's only waits: F(G) for its group's last panel, as W(j) had
                assert rec[o["wait0"]]["kind"] == PANEL and rec[o["wait0"]]["c1"] == o["k1"]
            if o["kind"] == T and o["wait0"] >= 0:
                assert rec[o["wait0"]]["kind"] == F
        if o["kind"] == PANEL:
            assert o["stream"] == CHAIN and o["wait0"] < 0 and o["wait1"] < 0
    sizes = group_sizes(ops)
    assert sizes[0] == 1 and max(sizes) <= gmax and sum(sizes) == len(pc) - 1
    if hide >= 1e12 and gmax > 1:          # every far update hides everything: 1, 2, 4, ... up to the maximum -- except that a
        want, left = [1], len(pc) - 2      # group never reaches the last panel (no far update runs beside such a group's chain)
        while left > 0:
            g = min(2 * want[-1], gmax, left)
            if g == left and g > 1:
                g -= 1
            want.append(g); left -= g
        assert sizes == want
    if hide == 0.0 or gmax == 1:
        assert set(sizes) == {1}
        # the one-level schedule: T = U(j, j+1) on the chain, F = W(j) = everything from panel j+2 on
        for o in ops:
            if o["kind"] in (T, F):
                j = pc.index(o["k0"])
                assert o["k1"] == pc[j + 1] and o["c0"] == pc[j + 1 + (o["kind"] == F)]
        assert not [o for o in ops if o["kind"] == L]


def test_cut_back_cases_mix_group_sizes():
    """the intermediate margins above do produce what they are there for: groups that grow and are cut back again"""
    seen = set()
    for case in CASES:
        if 0.0 < case[4] < 1e12:
            sizes = group_sizes(get_plan(*case)[1])
            print(case, sizes)
            seen |= set(sizes)
            assert max(sizes) > 1 and sizes[-1] == 1
    assert len(seen) >= 3


def test_plan_rejects_bad_sizes():
    from george_amd import _native as N
    ns, no = C.c_int32(0), C.c_int32(0)
    for bad in ((1000, 256, 0, 2), (2048, 100, 0, 2), (2048, 256, 0, 0), (0, 256, 0, 2)):
        with pytest.raises(ValueError):
            N.check(N.lib.gh_debug_chol_plan(bad[0], bad[1], bad[2], bad[3], 0.0, None, 0, C.byref(ns), None, 0, C.byref(no), None))
