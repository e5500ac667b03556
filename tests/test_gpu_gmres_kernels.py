"""The five vector kernels of ehyb_gmres one launch at a time through ehyb_gmres_*_step, bit for bit, on the inputs of
gmres_cases.py: every output is one number in fp64, so every vector, every basis column, every single partial and every double of
the tail is compared exactly (up to the sign of zero).  No tolerance appears in this file.

Guards of every test: each device vector has a pad of PAD doubles behind n, the basis a pad behind its last column, the slot array
a pad behind the tail; they must keep their sentinel, and so must every output a kernel does not write, every slot it does not
name, entries 512..1023 of the slots it writes and every double of the tail it does not name.  Entries 512..1023 of the slots a
kernel READS hold NaN.  Inputs come back unchanged.  The basis is uploaded with leading dimension n rounded up to even; for an odd
n the padding element of every column holds the sentinel: no kernel may read or write it."""
import ctypes as C

import numpy as np
import pytest

import gmres_cases as gc
import solver_cases as sc
from solver_cases import MAX_GRID, PAD, SENTINEL, STEP_GRID

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2
ITERS = 41


@pytest.fixture(scope="module")
def layout(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.GmresSlots()
    assert _lib.load().ehyb_gmres_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert out["slot_doubles"] == MAX_GRID and (out["status_running"], out["status_converged"], out["status_breakdown"]) == (RUNNING, CONVERGED, BREAKDOWN)
    return out


def same(got, want, what):
    """equal as numbers (0.0 == -0.0), NaN equal to NaN"""
    ok = np.array_equal(got, want, equal_nan=True)
    if not ok:
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: {len(bad)} differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


class Bench:
    """named device arrays with sentinel pads, the slot array with the tail, one launch, and the comparison of EVERYTHING"""

    def __init__(self, E, L, n, status=RUNNING, iters=ITERS, cycle=ITERS):
        self.E, self.L, self.n, self.lib = E, L, n, E.host._lib.load()
        self.ld = n + (n & 1)
        self.host, self.dev = {}, {}
        self.tail_at = L["slots"] * MAX_GRID
        self.s = np.full(self.tail_at + L["tail_doubles"] + PAD, SENTINEL)
        self.ints("flags_at", status, iters)
        self.ints("cycle_at", cycle, 0)

    def ints(self, at, a, b, target=None):
        f = np.zeros(2, dtype=np.int32)
        if at == "flags_at":
            f[self.L["flag_status"]], f[self.L["flag_iters"]] = a, b
        else:
            f[:] = a, b
        (self.s if target is None else target)[self.tail_at + self.L[at]] = f.view(np.float64)[0]

    def tail(self, at, values, target=None, offset=0):
        v = np.atleast_1d(np.asarray(values, dtype=np.float64))
        t = self.s if target is None else target
        t[self.tail_at + self.L[at] + offset:self.tail_at + self.L[at] + offset + len(v)] = v
        return self

    def upload(self, name, h):
        self.host[name] = h
        self.dev[name] = self.E.DeviceBuffer(len(h)).upload(h)
        return self

    def vec(self, name, values=None):
        h = np.full(self.n + PAD, SENTINEL)
        if values is not None:
            h[:self.n] = values.f(name) if isinstance(values, sc.Fx) else values
        return self.upload(name, h)

    def basis(self, columns, total):
        """`total` columns of leading dimension ld: the given ones, then sentinels"""
        h = np.full(self.ld * total + PAD, SENTINEL)
        for i, v in enumerate(columns):
            h[i * self.ld:i * self.ld + self.n] = v.f(f"v{i}")
        return self.upload("V", h)

    def slot(self, which, values):
        self.s[which * MAX_GRID:(which + 1) * MAX_GRID] = values
        return self

    def plant(self, which, fraction, seed=0):
        f = gc.fx_of(fraction)
        return self.slot(which, sc.planted_slot(f.m, e=f.e, seed=seed))

    def call(self, fn, *args):
        if "slots" not in self.dev:
            self.upload("slots", self.s.copy())
        conv = [C.c_void_p(self.dev[a].ptr) if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, fn)(self.n, *conv, None)
        assert rc == 0, (fn, rc, self.lib.ehyb_last_error())
        assert self.lib.ehyb_dev_sync() == 0, (fn, self.lib.ehyb_last_error())

    def expect(self, what, vectors=(), columns=(), slots=(), tail=(), flags=None):
        """everything on the device against what was uploaded, but for: vectors name -> [0, n), columns i -> basis column i,
        slots which -> the first STEP_GRID entries, tail (name, offset) -> values, flags (status, iters)"""
        h = self.host["slots"]
        for name, new in dict(vectors).items():
            self.host[name][:self.n] = new.f(name) if isinstance(new, sc.Fx) else new
        for i, new in dict(columns).items():
            self.host["V"][i * self.ld:i * self.ld + self.n] = new.f(f"v{i}")
        for which, new in dict(slots).items():
            h[which * MAX_GRID:which * MAX_GRID + STEP_GRID] = new.f(f"slot {which}") if isinstance(new, sc.Fx) else new
        for (at, offset), values in dict(tail).items():
            self.tail(at, values, target=h, offset=offset)
        if flags is not None:
            self.ints("flags_at", *flags, target=h)
        for name, want in self.host.items():
            got = self.dev[name].download()
            if name == "slots":
                want = want.copy()
                for k in range(self.L["slots"]):
                    same(got[k * MAX_GRID:(k + 1) * MAX_GRID], want[k * MAX_GRID:(k + 1) * MAX_GRID], f"{what}: slot {k}")
                ints = [self.tail_at + self.L["flags_at"], self.tail_at + self.L["cycle_at"]]
                for at in ints:
                    assert tuple(got[at:at + 1].view(np.int32)) == tuple(want[at:at + 1].view(np.int32)), (what, "ints at", at - self.tail_at, got[at:at + 1].view(np.int32))
                    got[at] = want[at] = 0.0
                same(got[self.tail_at:], want[self.tail_at:], f"{what}: the tail and its pad")
            else:
                same(got, want, f"{what}: {name}")


def c_slot(L, i):
    return L["slot_c0"] + i


# ------------------------------------------------------------------ start
@pytest.mark.parametrize("n", gc.SIZES)
def test_start_step(E, gpu, layout, n):
    L = layout
    c = gc.start_case(n, seed=n % 97)
    b = Bench(E, L, n).vec("b", c["in"]["b"]).vec("w", c["in"]["w"])
    b.call("ehyb_gmres_start_step", "b", "w", "slots")
    b.expect(f"start n={n}", {"w": c["out"]["w"]}, slots={L["slot_ww"]: c["sums"]["ww"], L["slot_bb"]: c["sums"]["bb"]})


# ------------------------------------------------------------------ dots
@pytest.mark.parametrize("count", gc.COUNTS)
@pytest.mark.parametrize("n", gc.SIZES)
def test_dots_step(E, gpu, layout, n, count):
    L = layout
    c = gc.dots_case(n, count, seed=n % 89 + count)
    b = Bench(E, L, n).vec("w", c["w"]).basis(c["V"], count)
    b.call("ehyb_gmres_dots_step", b.ld, "V", "w", count, "slots")
    b.expect(f"dots n={n} count={count}", slots={c_slot(L, i): p for i, p in enumerate(c["sums"])})


# ------------------------------------------------------------------ update
def update_bench(E, L, n, count, last, pass_, seed, status=RUNNING):
    c = gc.update_case(n, count, last, seed=seed)
    b = Bench(E, L, n, status=status).vec("w", c["w"]).basis(c["V"], count)
    for i, ci in enumerate(c["c"]):
        b.plant(c_slot(L, i), ci, seed=i)
    prev = [gc.DYADICS[(i + 3) % len(gc.DYADICS)] * 2 for i in range(count)]
    if pass_ == 1:
        b.tail("h_at", [float(v) for v in prev])
    want_h = [gc.exact(ci + (prev[i] if pass_ == 1 else 0)) for i, ci in enumerate(c["c"])]
    return c, b, want_h


@pytest.mark.parametrize("count", gc.COUNTS)
@pytest.mark.parametrize("n", gc.SIZES)
def test_update_step(E, gpu, layout, n, count):
    """pass 0 without the sum of squares and pass 1 with it: w, the Hessenberg copy of the pass, and on the last pass w.w"""
    L = layout
    for pass_, last in ((0, 0), (1, 1), (0, 1)):
        c, b, want_h = update_bench(E, L, n, count, last, pass_, n % 83 + count + pass_)
        b.call("ehyb_gmres_update_step", b.ld, "V", "w", count, "slots", pass_, last)
        b.expect(f"update n={n} count={count} pass={pass_} last={last}", {"w": c["w_new"]},
                 slots={L["slot_ww"]: c["ww"]} if last else {}, tail={("h_at", pass_ * L["h_stride"]): want_h})


# ------------------------------------------------------------------ next
THR = 2.0 ** -40                 # rho = (6/5)^2 and b.b = 4: far from converged


def next_bench(E, L, n, j, with_dinv, seed, passes=2, status=RUNNING, bb=4.0):
    c = gc.next_case(n, j, with_dinv, seed=seed)
    b = Bench(E, L, n, status=status).vec("w", c["w"]).vec("z").basis([], j + 2)
    if with_dinv:
        b.vec("dinv", c["dinv"])
    b.plant(L["slot_ww"], c["ww"], seed=3)
    b.tail("h_at", c["h"], offset=(passes - 1) * L["h_stride"])
    b.tail("cs_at", [r[0] for r in c["rot"]]).tail("sn_at", [r[1] for r in c["rot"]])
    b.tail("gt_at", c["gt"], offset=j).tail("bb_at", bb)
    return c, b


def next_args(b, with_dinv, j, passes, thr):
    return (b.ld, "V", "w", "dinv" if with_dinv else None, "z", "slots", j, passes, thr)


def next_tail(c, j):
    return {("r_at", j * 64): c["R"], ("cs_at", j): c["cs"], ("sn_at", j): c["sn"], ("g_at", j): c["g"], ("gt_at", j + 1): c["gt_next"],
            ("rho_at", 0): c["rho"]}


@pytest.mark.parametrize("j", [0, 1, 2, 7, 8, 30, 63])
@pytest.mark.parametrize("n", gc.SIZES)
def test_next_step(E, gpu, layout, n, j):
    """the column, the rotation, g, rho, the counter; v_{j+1} = w / h_{j+1} and z = M^-1 v_{j+1}; the status stays"""
    L = layout
    assert L["r_stride"] == 64
    for with_dinv, passes in ((False, 2), (True, 1)):
        c, b = next_bench(E, L, n, j, with_dinv, n % 79 + j, passes=passes)
        b.call("ehyb_gmres_next_step", *next_args(b, with_dinv, j, passes, THR))
        b.expect(f"next n={n} j={j} inv_diag={with_dinv}", {"z": c["z"]}, columns={j + 1: c["v"]}, tail=next_tail(c, j), flags=(RUNNING, ITERS + 1))


@pytest.mark.parametrize("n", gc.SIZES)
def test_next_step_at_the_cycle_start(E, gpu, layout, n):
    """j = -1: beta = sqrt(r.r) = 3/2; v_0, z, g~_0, rho, bb and the counter at the cycle start; b.b = 0 counts as 1"""
    L = layout
    for with_dinv, bb in ((False, 4), (True, 0)):
        c = gc.first_case(n, with_dinv, seed=n % 73)
        b = Bench(E, L, n, cycle=7).vec("w", c["w"]).vec("z").basis([], 1)
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.plant(L["slot_ww"], c["ww"], seed=4).slot(L["slot_bb"], sc.planted_slot(bb, seed=6))
        b.call("ehyb_gmres_next_step", *next_args(b, with_dinv, -1, 2, THR))
        b.ints("cycle_at", ITERS, 0, target=b.host["slots"])
        b.expect(f"first n={n} inv_diag={with_dinv}", {"z": c["z"]}, columns={0: c["v"]},
                 tail={("gt_at", 0): c["beta"], ("rho_at", 0): float(c["ww"]), ("bb_at", 0): float(bb) if bb else 1.0})


def test_next_converges_and_breaks_down(E, gpu, layout):
    """rho <= thr bb exactly: the step counts, its column is written, the status is converged and no vector moves; one ulp
    less: it goes on.  A NaN in the column or a zero gamma: breakdown, nothing but the status.  At the cycle start: r.r <= thr bb
    converged, a NaN in r.r or b.b breakdown, with rho and bb noted."""
    L, n, j = layout, 257, 2
    c, b = next_bench(E, L, n, j, True, 5)
    thr = c["rho"] / 4.0
    b.call("ehyb_gmres_next_step", *next_args(b, True, j, 2, thr))
    b.expect("converged at equality", tail=next_tail(c, j), flags=(CONVERGED, ITERS + 1))
    c, b = next_bench(E, L, n, j, True, 5)
    b.call("ehyb_gmres_next_step", *next_args(b, True, j, 2, np.nextafter(thr, 0.0)))
    b.expect("one ulp below", {"z": c["z"]}, columns={j + 1: c["v"]}, tail=next_tail(c, j), flags=(RUNNING, ITERS + 1))
    for what in ("nan-h", "nan-ww", "zero-gamma"):
        c, b = next_bench(E, L, n, j, True, 5)
        if what == "nan-h":
            b.tail("h_at", np.nan, offset=L["h_stride"] + 1)
        elif what == "nan-ww":
            b.slot(L["slot_ww"], sc.planted_slot(0, seed=1) + np.where(np.arange(MAX_GRID) == 3, np.nan, 0.0))
        else:
            b.tail("h_at", np.zeros(j + 1), offset=L["h_stride"]).slot(L["slot_ww"], sc.planted_slot(0, seed=1))
        b.call("ehyb_gmres_next_step", *next_args(b, True, j, 2, THR))
        b.expect(f"breakdown {what}", flags=(BREAKDOWN, ITERS))
    for what, ww, bb, status in (("converged", 9, 4, CONVERGED), ("nan-rr", np.nan, 4, BREAKDOWN), ("nan-bb", 9, np.nan, BREAKDOWN)):
        c = gc.first_case(n, False, seed=1)
        b = Bench(E, L, n, cycle=7).vec("w", c["w"]).vec("z").basis([], 1)
        for which, total in ((L["slot_ww"], ww), (L["slot_bb"], bb)):
            b.slot(which, sc.planted_slot(0 if np.isnan(total) else total, seed=2) + (np.where(np.arange(MAX_GRID) == 5, np.nan, 0.0) if np.isnan(total) else 0.0))
        b.call("ehyb_gmres_next_step", *next_args(b, False, -1, 2, 9.0 / 4.0))
        b.ints("cycle_at", ITERS, 0, target=b.host["slots"])
        b.expect(f"cycle start {what}", tail={("rho_at", 0): float(ww), ("bb_at", 0): float(bb)}, flags=(status, ITERS))


# ------------------------------------------------------------------ solve_x
@pytest.mark.parametrize("J", [1, 2, 8, 9, 31, 64])
@pytest.mark.parametrize("n", gc.SIZES)
def test_solve_x_step(E, gpu, layout, n, J):
    """R y = g, x += M^-1 V y over the J steps counted since the cycle start; whatever the status"""
    L = layout
    for with_dinv, status in ((False, RUNNING), (True, CONVERGED)):
        c = gc.solve_x_case(n, J, with_dinv, seed=n % 71 + J)
        b = Bench(E, L, n, status=status, iters=ITERS + J, cycle=ITERS).vec("x", c["x"]).basis(c["V"], J)
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.tail("g_at", c["g"])
        for col in range(J):
            b.tail("r_at", [c["R"][i][col] for i in range(col + 1)], offset=col * L["r_stride"])
        b.call("ehyb_gmres_solve_x_step", b.ld, "V", "dinv" if with_dinv else None, "x", "slots")
        b.expect(f"solve_x n={n} J={J} inv_diag={with_dinv}", {"x": c["x_new"]})


def test_solve_x_without_a_counted_step_writes_nothing(E, gpu, layout):
    L, n = layout, 257
    c = gc.solve_x_case(n, 3, True, seed=1)
    for iters, cycle in ((ITERS, ITERS), (ITERS, ITERS + 2)):
        b = Bench(E, L, n, iters=iters, cycle=cycle).vec("x", c["x"]).vec("dinv", c["dinv"]).basis(c["V"], 3)
        b.call("ehyb_gmres_solve_x_step", b.ld, "V", "dinv", "x", "slots")
        b.expect(f"solve_x iters={iters} cycle={cycle}")


# ------------------------------------------------------------------ a set status
@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
def test_steps_return_at_once_when_the_status_is_set(E, gpu, layout, status):
    """the inputs of the value tests, on which each step would write: with the status set nothing moves"""
    L = layout
    for n in (257, gc.SIZES[-1]):
        c = gc.start_case(n, seed=3)
        b = Bench(E, L, n, status=status).vec("b", c["in"]["b"]).vec("w", c["in"]["w"])
        b.call("ehyb_gmres_start_step", "b", "w", "slots")
        b.expect(f"start with status {status}")
        c = gc.dots_case(n, 9, seed=4)
        b = Bench(E, L, n, status=status).vec("w", c["w"]).basis(c["V"], 9)
        b.call("ehyb_gmres_dots_step", b.ld, "V", "w", 9, "slots")
        b.expect(f"dots with status {status}")
        c, b, _ = update_bench(E, L, n, 9, 1, 1, 5, status=status)
        b.call("ehyb_gmres_update_step", b.ld, "V", "w", 9, "slots", 1, 1)
        b.expect(f"update with status {status}")
        c, b = next_bench(E, L, n, 8, True, 6, status=status)
        b.call("ehyb_gmres_next_step", *next_args(b, True, 8, 2, THR))
        b.expect(f"next with status {status}")
