"""The solvers' vector kernels one launch at a time, bit for bit: the four CG kernels through ehyb_cg_*_step, the six
BiCGSTAB kernels through ehyb_bicgstab_*_step, on the inputs of solver_cases.py -- every output is one number in fp64
whatever the order of summation, so every vector and every single partial is compared exactly (up to the sign of zero),
at sizes chosen from the kernels' index walk (solver_cases.SIZES: every profile of unrolled and tail trips).  Then the
wide CG kernels (K = 2..4, frozen columns, ldx > n) where their unrolled bodies run, and the solves as the composition of
the tested kernels.  No tolerance appears in this file.

Guards of every step test: each device vector has a pad of PAD doubles behind n that must keep its sentinel; so must the
outputs a kernel does not write, every slot it does not name and entries 512..1023 of the slots it writes; entries
512..1023 of the slots a kernel READS hold NaN (partials_of must add gridDim.x entries and no more); inputs come back
unchanged."""
import ctypes as C
import math

import numpy as np
import pytest

import solver_cases as sc
from solver_cases import MAX_GRID, PAD, S, SENTINEL, STEP_GRID
from test_gpu_bicgstab import cd_matrix
from test_gpu_cg import spd_matrix

pytestmark = pytest.mark.gpu

THR = 0.75                    # rtol^2 of the BiCGSTAB step tests; with s.s = 3 and b.b = 4 planted, s.s == thr * b.b exactly
RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2


def assert_same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got == want) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        bad = np.flatnonzero(~ok)
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} entries differ; entry {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")


@pytest.fixture(scope="module")
def cg_layout(E):
    v = [C.c_int() for _ in range(6)]
    assert E.host._lib.load().ehyb_cg_layout(*(C.byref(a) for a in v)) == 0
    out = dict(zip(("slots", "slot_doubles", "bb", "pq", "rr", "rz0"), (a.value for a in v)))
    assert out["slot_doubles"] == MAX_GRID and out["slots"] == 5
    assert sorted((out["bb"], out["pq"], out["rz0"], out["rr"], out["rz0"] + 2)) == list(range(5)) and out["rr"] == out["rz0"] + 1
    return out


@pytest.fixture(scope="module")
def bi_layout(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.BicgstabSlots()
    assert _lib.load().ehyb_bicgstab_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert out["slot_doubles"] == MAX_GRID and out["slots"] == 8 and out["flag_count"] == 2
    named = [out[k] for k in ("slot_bb", "slot_rv", "slot_ss", "slot_ts", "slot_tt", "slot_rho0", "slot_rr")] + [out["slot_rho0"] + 2]
    assert sorted(named) == list(range(8)) and out["slot_rr"] == out["slot_rho0"] + 1
    assert (out["flag_status"], out["flag_iters"]) == (0, 1)
    assert (out["status_running"], out["status_converged"], out["status_breakdown"]) == (RUNNING, CONVERGED, BREAKDOWN)
    assert _lib.load().ehyb_bicgstab_layout(None) != 0
    return out


class Bench:
    """The device side of one step test: named vectors of n doubles with a sentinel pad, the slot array (with the flags
    of BiCGSTAB behind it and a pad behind those), one launch, and the comparison of EVERYTHING with what is expected."""

    def __init__(self, E, n, slots, flags=None):
        self.E, self.n, self.lib = E, n, E.host._lib.load()
        self.host, self.dev = {}, {}
        self.n_slots = slots
        self.s = np.full(slots * MAX_GRID + (1 if flags is not None else 0) + PAD, SENTINEL)
        self.flag_at = slots * MAX_GRID
        if flags is not None:
            self.set_flags(*flags)

    def vec(self, name, values=None):
        """a device vector: the n values (an Fx, floats, or None = sentinels: an output) and the pad"""
        h = np.full(self.n + PAD, SENTINEL)
        if values is not None:
            h[:self.n] = values.f(name) if isinstance(values, sc.Fx) else values
        self.host[name] = h
        self.dev[name] = self.E.DeviceBuffer(len(h)).upload(h)
        return self

    def vecs(self, mapping):
        for k, v in mapping.items():
            self.vec(k, v)
        return self

    def slot(self, which, values):
        self.s[which * MAX_GRID:(which + 1) * MAX_GRID] = values
        return self

    def set_flags(self, status, iters):
        self.s[self.flag_at] = np.array([status, iters], dtype=np.int32).view(np.float64)[0]

    def upload_slots(self):
        self.dev["slots"] = self.E.DeviceBuffer(len(self.s)).upload(self.s)
        self.host["slots"] = self.s.copy()

    def call(self, fn, *args):
        """fn(n, ...) with names turned into device pointers ("slots": the slot array), None and numbers as they are"""
        if "slots" not in self.dev:
            self.upload_slots()
        conv = [C.c_void_p(self.dev[a].ptr) if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, fn)(self.n, *conv, None)
        assert rc == 0, (fn, rc, self.lib.ehyb_last_error())
        assert self.lib.ehyb_dev_sync() == 0, (fn, self.lib.ehyb_last_error())

    def flags(self):
        return tuple(int(v) for v in self.dev["slots"].download()[self.flag_at:self.flag_at + 1].view(np.int32))

    def expect(self, what, vectors=(), slots=(), flags=None):
        """Everything on the device against the uploaded state, but for: vectors name -> new values of [0, n), slots
        which -> the first STEP_GRID entries, flags (status, iters).  The expected state becomes the new baseline."""
        for name, new in dict(vectors).items():
            self.host[name][:self.n] = new.f(name) if isinstance(new, sc.Fx) else new
        for which, new in dict(slots).items():
            self.host["slots"][which * MAX_GRID:which * MAX_GRID + STEP_GRID] = new.f(f"slot {which}") if isinstance(new, sc.Fx) else new
        if flags is not None:
            self.host["slots"][self.flag_at] = np.array(flags, dtype=np.int32).view(np.float64)[0]
            assert self.flags() == tuple(flags), (what, self.flags(), flags)
        for name, h in self.host.items():
            got = self.dev[name].download()
            if name == "slots":
                for k in range(self.n_slots):
                    assert_same(got[k * MAX_GRID:(k + 1) * MAX_GRID], h[k * MAX_GRID:(k + 1) * MAX_GRID], f"{what}: slot {k}")
                assert np.array_equal(got[self.flag_at:].view(np.int64), h[self.flag_at:].view(np.int64)), f"{what}: flags or the pad behind the slots"
            else:
                assert_same(got[:self.n], h[:self.n], f"{what}: {name}")
                assert np.array_equal(got[self.n:].view(np.int64), h[self.n:].view(np.int64)), f"{what}: the pad behind {name}"


def planted(case, name, seed=0):
    num, den = case["scalars"][name]
    assert den == 1
    return sc.planted_slot(num, seed=seed)


def special_slot(value, second=0.0):
    """a slot whose sum is `value` (a zero, an infinity, a NaN, a huge or a tiny number): one entry, the others zero"""
    out = np.full(MAX_GRID, np.nan)
    out[:STEP_GRID] = 0.0
    out[137] = value
    out[401] = second
    return out


def variants(n):
    """(cur, with inv_diag) of a step test"""
    return [(cur, d) for cur in (0, 1) for d in (False, True)]


# ------------------------------------------------------------------ CG: the ehyb_cg_*_step entry points (K = 1)
@pytest.mark.parametrize("n", sc.SIZES)
def test_cg_init_step(E, gpu, cg_layout, n):
    sc.asserted_walk(n)
    L = cg_layout
    for with_dinv in (False, True):
        c = sc.cg_init_case(n, with_dinv, seed=n % 97)
        b = Bench(E, n, L["slots"]).vecs(c["in"]).vec("r").vec("p")
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.call("ehyb_cg_init_step", "b", "q", "dinv" if with_dinv else None, "r", "p", "slots")
        b.expect(f"cg init n={n} inv_diag={with_dinv}", c["out"],
                 {L["rz0"]: c["sums"]["rz"], L["rr"]: c["sums"]["rr"], L["bb"]: c["sums"]["bb"]})


@pytest.mark.parametrize("n", sc.SIZES)
def test_cg_dot_step(E, gpu, cg_layout, n):
    sc.asserted_walk(n)
    c = sc.dot_case(n, seed=n % 89)
    b = Bench(E, n, cg_layout["slots"]).vecs(c["in"])
    b.call("ehyb_cg_dot_step", "p", "q", "slots")
    b.expect(f"cg dot n={n}", {}, {cg_layout["pq"]: c["sums"]["pq"]})


def cg_update_bench(E, L, n, cur, with_dinv, seed):
    c = sc.cg_update_case(n, cur, with_dinv, seed=seed)
    b = Bench(E, n, L["slots"]).vecs(c["in"])
    if with_dinv:
        b.vec("dinv", c["dinv"])
    b.slot(L["rz0"] + 2 * cur, planted(c, "rz", 1)).slot(L["pq"], planted(c, "pq", 2))
    return c, b


@pytest.mark.parametrize("n", sc.SIZES)
def test_cg_update_step(E, gpu, cg_layout, n):
    sc.asserted_walk(n)
    L = cg_layout
    for cur, with_dinv in variants(n):
        c, b = cg_update_bench(E, L, n, cur, with_dinv, n % 83 + cur)
        b.call("ehyb_cg_update_step", "p", "q", "dinv" if with_dinv else None, "x", "r", "slots", cur)
        b.expect(f"cg update n={n} cur={cur} inv_diag={with_dinv}", c["out"],
                 {L["rz0"] + 2 * (cur ^ 1): c["sums"]["rz"], L["rr"]: c["sums"]["rr"]})


def cg_direction_bench(E, L, n, cur, with_dinv, seed):
    c = sc.cg_direction_case(n, cur, with_dinv, seed=seed)
    b = Bench(E, n, L["slots"]).vecs(c["in"])
    if with_dinv:
        b.vec("dinv", c["dinv"])
    b.slot(L["rz0"] + 2 * (cur ^ 1), planted(c, "rz_new", 3)).slot(L["rz0"] + 2 * cur, planted(c, "rz", 4))
    return c, b


@pytest.mark.parametrize("n", sc.SIZES)
def test_cg_direction_step(E, gpu, cg_layout, n):
    sc.asserted_walk(n)
    for cur, with_dinv in variants(n):
        c, b = cg_direction_bench(E, cg_layout, n, cur, with_dinv, n % 79 + cur)
        b.call("ehyb_cg_direction_step", "r", "dinv" if with_dinv else None, "p", "slots", cur)
        b.expect(f"cg direction n={n} cur={cur} inv_diag={with_dinv}", c["out"])


def test_cg_cur_is_masked(E, gpu, cg_layout):
    n = 3 * S + 1
    for passed in (2, 3):
        c, b = cg_update_bench(E, cg_layout, n, passed & 1, True, 5)
        b.call("ehyb_cg_update_step", "p", "q", "dinv", "x", "r", "slots", passed)
        b.expect(f"cg update cur={passed}", c["out"], {cg_layout["rz0"] + 2 * ((passed & 1) ^ 1): c["sums"]["rz"], cg_layout["rr"]: c["sums"]["rr"]})
        c, b = cg_direction_bench(E, cg_layout, n, passed & 1, True, 6)
        b.call("ehyb_cg_direction_step", "r", "dinv", "p", "slots", passed)
        b.expect(f"cg direction cur={passed}", c["out"])


@pytest.mark.parametrize("probe", sc.DIVISION_PROBES, ids=[f"probe{i}" for i in range(len(sc.DIVISION_PROBES))])
def test_cg_scalars_are_correctly_rounded_quotients(E, gpu, cg_layout, probe):
    """alpha = r.z / p.q read back as x = fma(alpha, 1, 0), beta = r.z_new / r.z as p = fma(beta, 1, 0)"""
    L, n, (R, P) = cg_layout, 257, probe
    want = np.full(n, sc.rounded_quotient(R, P))
    for cur in (0, 1):
        b = Bench(E, n, L["slots"]).vecs({"p": np.ones(n), "q": np.zeros(n), "x": np.zeros(n), "r": np.zeros(n)})
        b.slot(L["rz0"] + 2 * cur, sc.planted_slot(R, seed=5)).slot(L["pq"], sc.planted_slot(P, seed=6))
        b.call("ehyb_cg_update_step", "p", "q", None, "x", "r", "slots", cur)
        b.expect(f"alpha = {R} / {P}", {"x": want, "r": np.zeros(n)}, {L["rz0"] + 2 * (cur ^ 1): np.zeros(STEP_GRID), L["rr"]: np.zeros(STEP_GRID)})
        b = Bench(E, n, L["slots"]).vecs({"r": np.zeros(n), "p": np.ones(n)})
        b.slot(L["rz0"] + 2 * (cur ^ 1), sc.planted_slot(R, seed=7)).slot(L["rz0"] + 2 * cur, sc.planted_slot(P, seed=8))
        b.call("ehyb_cg_direction_step", "r", None, "p", "slots", cur)
        b.expect(f"beta = {R} / {P}", {"p": want})


# ------------------------------------------------------------------ BiCGSTAB: the ehyb_bicgstab_*_step entry points
def rho_slot(L, c):
    return L["slot_rho0"] + 2 * c


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_init_step(E, gpu, bi_layout, n):
    sc.asserted_walk(n)
    L = bi_layout
    for with_dinv in (False, True):
        c = sc.bicg_init_case(n, with_dinv, seed=n % 97)
        b = Bench(E, n, L["slots"], flags=(RUNNING, 41)).vecs(c["in"]).vec("r").vec("rh").vec("p")
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.call("ehyb_bicgstab_init_step", "b", "q", "dinv" if with_dinv else None, "r", "rh", "p", "slots")
        b.expect(f"bicgstab init n={n} inv_diag={with_dinv}", c["out"],
                 {rho_slot(L, 0): c["sums"]["rho"], L["slot_rr"]: c["sums"]["rr"], L["slot_bb"]: c["sums"]["bb"]}, flags=(RUNNING, 41))


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_dot_and_dot2_steps(E, gpu, bi_layout, n):
    sc.asserted_walk(n)
    L = bi_layout
    c = sc.dot_case(n, seed=n % 89 + 1)
    b = Bench(E, n, L["slots"], flags=(RUNNING, 7)).vecs({"rh": c["in"]["p"], "v": c["in"]["q"]})
    b.call("ehyb_bicgstab_dot_step", "rh", "v", "slots")
    b.expect(f"bicgstab dot n={n}", {}, {L["slot_rv"]: c["sums"]["pq"]}, flags=(RUNNING, 7))
    c = sc.bicg_dot2_case(n, seed=n % 89 + 2)
    b = Bench(E, n, L["slots"], flags=(RUNNING, 7)).vecs(c["in"])
    b.call("ehyb_bicgstab_dot2_step", "t", "sv", "slots")
    b.expect(f"bicgstab dot2 n={n}", {}, {L["slot_ts"]: c["sums"]["ts"], L["slot_tt"]: c["sums"]["tt"]}, flags=(RUNNING, 7))


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_s_step(E, gpu, bi_layout, n):
    sc.asserted_walk(n)
    L = bi_layout
    for cur, with_dinv in variants(n):
        c = sc.bicg_s_case(n, cur, with_dinv, seed=n % 83 + cur)
        b = Bench(E, n, L["slots"], flags=(RUNNING, 3)).vecs(c["in"]).vec("sv").vec("sh")
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.slot(rho_slot(L, cur), planted(c, "rho", 1)).slot(L["slot_rv"], planted(c, "rv", 2))
        b.call("ehyb_bicgstab_s_step", "r", "v", "dinv" if with_dinv else None, "sv", "sh", "slots", cur)
        b.expect(f"bicgstab s n={n} cur={cur} inv_diag={with_dinv}", c["out"], {L["slot_ss"]: c["sums"]["ss"]}, flags=(RUNNING, 3))


def update_bench(E, L, n, cur, c, ss, bb, iters=41):
    """the update kernel's inputs: the case's vectors and scalars, s.s and b.b as whole slots"""
    b = Bench(E, n, L["slots"], flags=(RUNNING, iters)).vecs(c["in"]).vec("r")
    for name in ("sh", "t", "rh"):
        if name not in c["in"]:
            b.vec(name, np.full(n, 3.0))
    b.slot(rho_slot(L, cur), planted(c, "rho", 1)).slot(L["slot_rv"], planted(c, "rv", 2))
    b.slot(L["slot_ss"], ss).slot(L["slot_bb"], bb)
    if "ts" in c["scalars"]:
        b.slot(L["slot_ts"], planted(c, "ts", 3)).slot(L["slot_tt"], planted(c, "tt", 4))
    else:
        b.slot(L["slot_ts"], sc.planted_slot(5, seed=3)).slot(L["slot_tt"], sc.planted_slot(7, seed=4))
    return b


UPDATE_ARGS = ("p", "sh", "sv", "t", "rh", "x", "r", "slots")


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_update_step(E, gpu, bi_layout, n):
    """the full step: s.s = 7 > thr b.b = 3"""
    sc.asserted_walk(n)
    L = bi_layout
    for cur in (0, 1):
        c = sc.bicg_update_case(n, cur, seed=n % 83 + cur)
        b = update_bench(E, L, n, cur, c, sc.planted_slot(7, seed=5), sc.planted_slot(4, seed=6))
        b.call("ehyb_bicgstab_update_step", *UPDATE_ARGS, cur, THR)
        b.expect(f"bicgstab update n={n} cur={cur}", c["out"], {rho_slot(L, cur ^ 1): c["sums"]["rho"], L["slot_rr"]: c["sums"]["rr"]},
                 flags=(RUNNING, 42))


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_direction_step(E, gpu, bi_layout, n):
    """no stop: s.s = 7 and r.r = 9 against thr b.b = 3"""
    sc.asserted_walk(n)
    L = bi_layout
    for cur, with_dinv in variants(n):
        c = sc.bicg_direction_case(n, cur, with_dinv, seed=n % 79 + cur)
        b = Bench(E, n, L["slots"], flags=(RUNNING, 12)).vecs(c["in"])
        if with_dinv:
            b.vec("dinv", c["dinv"])
        for name, which in (("rho", rho_slot(L, cur)), ("rho_new", rho_slot(L, cur ^ 1)), ("rv", L["slot_rv"]), ("ts", L["slot_ts"]),
                            ("tt", L["slot_tt"])):
            b.slot(which, planted(c, name, which))
        b.slot(L["slot_ss"], sc.planted_slot(7, seed=5)).slot(L["slot_bb"], sc.planted_slot(4, seed=6)).slot(L["slot_rr"], sc.planted_slot(9, seed=7))
        b.call("ehyb_bicgstab_direction_step", "r", "v", "dinv" if with_dinv else None, "p", "slots", cur, THR)
        b.expect(f"bicgstab direction n={n} cur={cur} inv_diag={with_dinv}", c["out"], flags=(RUNNING, 12))


def test_bicgstab_cur_is_masked(E, gpu, bi_layout):
    L, n = bi_layout, 3 * S + 1
    for passed in (2, 3):
        cur = passed & 1
        c = sc.bicg_update_case(n, cur, seed=9)
        b = update_bench(E, L, n, cur, c, sc.planted_slot(7, seed=5), sc.planted_slot(4, seed=6))
        b.call("ehyb_bicgstab_update_step", *UPDATE_ARGS, passed, THR)
        b.expect(f"bicgstab update cur={passed}", c["out"], {rho_slot(L, cur ^ 1): c["sums"]["rho"], L["slot_rr"]: c["sums"]["rr"]}, flags=(RUNNING, 42))


ULP_ABOVE_3 = special_slot(3.0, 2.0 ** -51)      # 3 + one ulp, exact in every order (two non-zero entries)


@pytest.mark.parametrize("n", sc.SIZES)
def test_bicgstab_half_step(E, gpu, bi_layout, n):
    """s.s == thr * b.b exactly (3, 4 and 0.75; and 3/4 against a planted b.b = 0, which counts as 1): update takes the half
    step -- x += alpha p^, r = s, the partials of r.r, counter + 1, the rho slot and the status untouched -- and direction
    then sets converged and writes nothing else.  One ulp more s.s: the full step."""
    sc.asserted_walk(n)
    L = bi_layout
    for cur in (0, 1):
        for ss, bb in ((sc.planted_slot(3, seed=5), sc.planted_slot(4, seed=6)), (sc.planted_slot(3, e=2, seed=7), sc.planted_slot(0, seed=8))):
            c = sc.bicg_half_case(n, cur, seed=n % 83 + cur)
            b = update_bench(E, L, n, cur, c, ss, bb).vec("v", np.full(n, 5.0))
            b.slot(rho_slot(L, cur ^ 1), sc.planted_slot(11, seed=9, rest=SENTINEL))
            b.call("ehyb_bicgstab_update_step", *UPDATE_ARGS, cur, THR)
            b.expect(f"half step n={n} cur={cur}", c["out"], {L["slot_rr"]: c["sums"]["rr"]}, flags=(RUNNING, 42))
            b.call("ehyb_bicgstab_direction_step", "r", "v", None, "p", "slots", cur, THR)
            b.expect(f"direction after the half step n={n} cur={cur}", flags=(CONVERGED, 42))
        c = sc.bicg_update_case(n, cur, seed=n % 83 + cur)
        b = update_bench(E, L, n, cur, c, ULP_ABOVE_3, sc.planted_slot(4, seed=6))
        b.call("ehyb_bicgstab_update_step", *UPDATE_ARGS, cur, THR)
        b.expect(f"one ulp above n={n} cur={cur}", c["out"], {rho_slot(L, cur ^ 1): c["sums"]["rho"], L["slot_rr"]: c["sums"]["rr"]},
                 flags=(RUNNING, 42))


ALL_VECTORS = ("r", "rh", "p", "v", "sv", "sh", "t", "x", "dinv")


def healthy_state(E, L, n, cur, status=RUNNING, seed=0):
    """Every vector and every slot of an iteration in flight, such that each of the five flagged steps would run to its
    end and write (the value tests above show that they do): s.s = 7, r.r = 9, b.b = 4 against THR, finite non-zero scalars."""
    rng = np.random.default_rng(seed)
    b = Bench(E, n, L["slots"], flags=(status, 41))
    for name in ALL_VECTORS:
        b.vec(name, rng.integers(1, 9, n).astype(np.float64) if name != "dinv" else np.full(n, 0.5))
    for which, total in ((L["slot_ss"], 7), (L["slot_rr"], 9), (L["slot_bb"], 4), (rho_slot(L, cur), 6 * sc.ODD_C),
                         (rho_slot(L, cur ^ 1), 15 * sc.ODD_C), (L["slot_rv"], 16 * sc.ODD_C), (L["slot_ts"], 3 * 7654321), (L["slot_tt"], 4 * 7654321)):
        b.slot(which, sc.planted_slot(total, seed=which))
    return b


def launch_step(b, step, cur):
    args = {"dot": ("rh", "v", "slots"), "s": ("r", "v", "dinv", "sv", "sh", "slots", cur), "dot2": ("t", "sv", "slots"),
            "update": UPDATE_ARGS + (cur, THR), "direction": ("r", "v", "dinv", "p", "slots", cur, THR)}[step]
    b.call(f"ehyb_bicgstab_{step}_step", *args)


FLAGGED_STEPS = ("dot", "s", "dot2", "update", "direction")
HUGE, TINY = 2.0 ** 1000, 2.0 ** -1000
# (step, slot name -> value of its sum (cur: the rho slot of parity cur, new: the other), ...): each must end in breakdown
BREAKDOWNS = [
    ("s", {"rv": 0.0}), ("s", {"rv": np.inf}), ("s", {"rv": np.nan}), ("s", {"rv": -0.0}),
    ("s", {"cur": np.inf}), ("s", {"cur": np.nan}), ("s", {"cur": HUGE, "rv": TINY}),
    ("update", {"tt": 0.0}), ("update", {"tt": np.inf}), ("update", {"tt": np.nan}),
    ("update", {"ts": np.inf}), ("update", {"ts": np.nan}), ("update", {"ts": HUGE, "tt": TINY}),
    ("direction", {"cur": 0.0}), ("direction", {"ts": 0.0}), ("direction", {"new": np.inf}), ("direction", {"new": np.nan}),
    ("direction", {"cur": np.inf}), ("direction", {"tt": 0.0}), ("direction", {"new": HUGE, "cur": TINY}),
]


def slot_by_name(L, cur, name):
    return {"cur": rho_slot(L, cur), "new": rho_slot(L, cur ^ 1)}.get(name) if name in ("cur", "new") else L["slot_" + name]


@pytest.mark.parametrize("case", range(len(BREAKDOWNS)), ids=[f"{s}-" + "-".join(f"{k}={v}" for k, v in p.items()) for s, p in BREAKDOWNS])
def test_bicgstab_breakdown_writes_the_status_and_nothing_else(E, gpu, bi_layout, case):
    L, n = bi_layout, 3 * S + 1
    step, plantings = BREAKDOWNS[case]
    cur = case & 1
    b = healthy_state(E, L, n, cur, seed=case)
    for name, value in plantings.items():
        b.slot(slot_by_name(L, cur, name), special_slot(value))
    launch_step(b, step, cur)
    b.expect(f"{step} with {plantings}", flags=(BREAKDOWN, 41))
    for later in FLAGGED_STEPS:
        launch_step(b, later, cur)
        b.expect(f"{later} after the breakdown in {step}", flags=(BREAKDOWN, 41))


def test_bicgstab_convergence_is_tested_before_breakdown(E, gpu, bi_layout):
    """direction: r.r <= thr b.b (3 against 0.75 * 4, and 1 against it) together with rho = 0 (and with a NaN rho_new) is
    converged, not breakdown"""
    L, n = bi_layout, 3 * S + 1
    for cur, rr, poison in ((0, 3, {"cur": 0.0}), (1, 1, {"cur": 0.0}), (0, 3, {"new": np.nan}), (1, 3, {"ts": 0.0})):
        b = healthy_state(E, L, n, cur, seed=cur)
        b.slot(L["slot_rr"], sc.planted_slot(rr, seed=2))
        for name, value in poison.items():
            b.slot(slot_by_name(L, cur, name), special_slot(value))
        launch_step(b, "direction", cur)
        b.expect(f"direction r.r={rr} {poison}", flags=(CONVERGED, 41))
    # and one ulp more r.r with rho = 0: the breakdown is seen
    b = healthy_state(E, L, n, 0).slot(L["slot_rr"], ULP_ABOVE_3).slot(rho_slot(L, 0), special_slot(0.0))
    launch_step(b, "direction", 0)
    b.expect("direction r.r one ulp above, rho = 0", flags=(BREAKDOWN, 41))


@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
def test_bicgstab_steps_return_at_once_when_the_status_is_set(E, gpu, bi_layout, status):
    L = bi_layout
    for n in (257, 4 * S + 1):
        for cur in (0, 1):
            b = healthy_state(E, L, n, cur, status=status, seed=n % 5)
            for step in FLAGGED_STEPS:
                launch_step(b, step, cur)
                b.expect(f"{step} with the status preset to {status}, n={n}", flags=(status, 41))


@pytest.mark.parametrize("probe", sc.DIVISION_PROBES, ids=[f"probe{i}" for i in range(len(sc.DIVISION_PROBES))])
def test_bicgstab_scalars_are_correctly_rounded_quotients(E, gpu, bi_layout, probe):
    """alpha = rho / rh.v read back as s[0] = fma(-alpha, -1, 0), omega = t.s / t.t as x = fma(omega, 1, fma(alpha, 0, 0)), and
    beta = (rho_new / rho) * (alpha / omega), three divisions and a product rounded in that order, as p^ = fma(beta, 1 - omega 0, 0)"""
    L, n, (R, P) = bi_layout, 257, probe
    q = np.full(n, sc.rounded_quotient(R, P))
    zero, one = np.zeros(n), np.ones(n)
    for cur in (0, 1):
        first = np.zeros(n)
        first[0] = 1.0
        b = Bench(E, n, L["slots"], flags=(RUNNING, 0)).vecs({"r": zero, "v": -first}).vec("sv").vec("sh")
        b.slot(rho_slot(L, cur), sc.planted_slot(R, seed=1)).slot(L["slot_rv"], sc.planted_slot(P, seed=2))
        b.call("ehyb_bicgstab_s_step", "r", "v", None, "sv", "sh", "slots", cur)
        ss = np.zeros(STEP_GRID)
        ss[0] = q[0] * q[0]             # one non-zero term, fma(alpha, alpha, 0): one rounding, the same fused or not
        b.expect(f"alpha = {R} / {P}", {"sv": q * first, "sh": q * first}, {L["slot_ss"]: ss}, flags=(RUNNING, 0))

        b = Bench(E, n, L["slots"], flags=(RUNNING, 0)).vecs({"p": zero, "sh": one, "sv": zero, "t": zero, "rh": zero, "x": zero}).vec("r")
        for which, total in ((rho_slot(L, cur), 3), (L["slot_rv"], 8), (L["slot_ss"], 7), (L["slot_bb"], 4), (L["slot_ts"], R), (L["slot_tt"], P)):
            b.slot(which, sc.planted_slot(total, seed=which))
        b.call("ehyb_bicgstab_update_step", *UPDATE_ARGS, cur, THR)
        b.expect(f"omega = {R} / {P}", {"x": q, "r": zero}, {rho_slot(L, cur ^ 1): np.zeros(STEP_GRID), L["slot_rr"]: np.zeros(STEP_GRID)},
                 flags=(RUNNING, 1))

        # beta from five planted integers, none of the quotients dyadic
        rho_new, rho, rv, ts, tt = R, P, 7 * sc.ODD_C, 11 * 7654321, 13 * 7654321
        b = Bench(E, n, L["slots"], flags=(RUNNING, 0)).vecs({"r": zero, "v": zero, "p": one})
        for which, total in ((rho_slot(L, cur), rho), (rho_slot(L, cur ^ 1), rho_new), (L["slot_rv"], rv), (L["slot_ts"], ts), (L["slot_tt"], tt),
                             (L["slot_ss"], 7), (L["slot_bb"], 4), (L["slot_rr"], 9)):
            b.slot(which, sc.planted_slot(total, seed=which))
        b.call("ehyb_bicgstab_direction_step", "r", "v", None, "p", "slots", cur, THR)
        b.expect(f"beta from {rho_new}, {rho}", {"p": np.full(n, sc.bicg_beta_rounded(rho_new, rho, rv, ts, tt))}, flags=(RUNNING, 0))


# ------------------------------------------------------------------ the wide CG kernels where their unrolled bodies run
FULL_NX, FULL_NY = 1024, 921          # n = 943,104: about the bench size; the walk has (1,3) and (2,0)
MIX_RTOL, MIX_ITERS, MIX_EVERY = 1e-6, 12, 2
# Column kinds of the mix.  "near e": b = A x*, x0 = x* + e u (u uniform in [-1, 1]); on this matrix the relative residual of
# such a start is about e * (3.4, 0.41, 0.13, 0.059) after 0, 2, 4, 6 iterations (a numpy CG of the same recurrences, with
# and without Jacobi), so e = 1e-6, 5e-6, 1.2e-5 cross MIX_RTOL at the check points 2, 4 and 6.  "zero": b = 0, frozen before
# the first iteration.  "random": a random b from x0 = 0 is at 0.1 after 12 iterations and runs to max_iter.
MIX_KINDS = [("near", 5e-6), ("zero", 0), ("random", 0), ("near", 1e-6), ("near", 1.2e-5), ("near", 5e-6), ("random", 0)]
BIG_SPD_KW = dict(lds_doubles=5120, direct=2, sym_pairs=0, cg_fused_dot=2)       # (test_gpu_cheb_full.py builds its val_f32 plan with them)


class BigSystem:
    def __init__(self, E, A, symmetric, **kw):
        self.A, self.n = A, A.shape[0]
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(A.indptr, A.indices, A.data, self.cfg, symmetric=symmetric)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.plan = E.Plan(self.m, self.cfg)
        self.plain_launches = E.Plan(self.m, E.make_config(graphs=2, **kw))
        self.inv_diag = E.vector_reorder(1.0 / A.diagonal(), self.perm)
        st = self.plan.stats
        assert st["sym_pairs"] == 0 and st["er_partials"] == 0, "plain storage"
        assert (self.plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
        assert sc.solver_grid(self.n) == STEP_GRID, "the solve and the step entry points launch the same grid"
        self.profiles = sc.walk_profile(self.n, sc.solver_grid(self.n))
        assert {(1, 3), (2, 0)} <= self.profiles, self.profiles
        self.singles = {}


@pytest.fixture(scope="module")
def big_spd(E, gpu):
    s = BigSystem(E, spd_matrix(FULL_NX, FULL_NY, 3000, 21), True, **BIG_SPD_KW)
    rng = np.random.default_rng(77)
    x_star = np.sin(np.arange(s.n) * 1e-3) + 1.5
    B, X0 = [], []
    for kind, e in MIX_KINDS:
        if kind == "near":
            B.append(s.A @ x_star)
            X0.append(x_star + e * rng.uniform(-1, 1, s.n))
        else:
            B.append(np.zeros(s.n) if kind == "zero" else rng.uniform(-1, 1, s.n))
            X0.append(np.zeros(s.n))
    s.B = np.stack([E.vector_reorder(b, s.perm) for b in B])
    s.X0 = np.stack([E.vector_reorder(x, s.perm) for x in X0])
    return s


def single_solves(s, jacobi, k):
    out = []
    for j in range(k):
        if (jacobi, j) not in s.singles:
            s.singles[jacobi, j] = s.plan.cg(s.B[j], x0=s.X0[j], max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY,
                                             inv_diag=s.inv_diag if jacobi else None)
        out.append(s.singles[jacobi, j])
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def assert_columns_same_bits(got, want, what):
    X, it, rel = got
    Xw, itw, relw = want
    assert np.array_equal(np.asarray(it), itw), (what, it, itw)
    assert np.array_equal(np.asarray(rel).view(np.int64), relw.view(np.int64)), (what, rel, relw)
    for j in range(len(Xw)):
        assert np.array_equal(X[j].view(np.int64), Xw[j].view(np.int64)), (what, j, np.abs(X[j] - Xw[j]).max())


def assert_the_mix(iters, what):
    iters = [int(i) for i in iters]
    between = {i for i in iters if 0 < i < MIX_ITERS}
    assert 0 in iters and MIX_ITERS in iters and len(between) >= 2, (what, iters)


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_wide_cg_kernels_at_full_size_equal_the_single_solve(E, gpu, big_spd, k, jacobi):
    """ehyb_pcg_multi against ehyb_pcg per column, bit for bit, where every thread runs the unrolled bodies (profiles (1,3)
    and (2,0)): column groups of 2 (k = 2, 5), 3 (k = 3, 5, 6, 7) and 4 (k = 4, 7); from k = 4 on a column frozen before the
    first iteration, two that freeze at different check points and one that runs to max_iter -- asserted from iters_done."""
    s = big_spd
    want = single_solves(s, jacobi, k)
    got = s.plan.cg_multi(s.B[:k], s.X0[:k], max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY, inv_diag=s.inv_diag if jacobi else None)
    assert_columns_same_bits(got, want, f"k={k} jacobi={jacobi}")
    if k >= 4:
        assert_the_mix(got[1], f"k={k} jacobi={jacobi}")
    if k == 7:
        assert_columns_same_bits(s.plain_launches.cg_multi(s.B[:k], s.X0[:k], max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY,
                                                           inv_diag=s.inv_diag if jacobi else None), want, f"graphs=2 k={k} jacobi={jacobi}")


@pytest.mark.parametrize("k", [5, 7])
def test_wide_cg_kernels_at_full_size_with_ldx(E, gpu, big_spd, k):
    s, n = big_spd, big_spd.n
    ldb, ldx = n + 37, n + 5
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = s.B[:k]
    Xb = np.full((k, ldx), SENTINEL)
    Xb[:, :n] = s.X0[:k]
    db, dx, dd = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel()), E.DeviceBuffer(n).upload(s.inv_diag)
    it, rel = (C.c_int * k)(), (C.c_double * k)()
    lib = E.host._lib.load()
    rc = lib.ehyb_pcg_multi(s.plan.h, C.c_void_p(dd.ptr), C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, MIX_ITERS, MIX_RTOL, MIX_EVERY,
                            None, it, rel)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(Xo[:, n:].view(np.int64), Xb[:, n:].view(np.int64)), "the gap behind the columns of X"
    assert np.array_equal(db.download().view(np.int64), Bb.ravel().view(np.int64))
    assert_columns_same_bits((Xo[:, :n], np.array(list(it)), np.array(list(rel))), single_solves(s, True, k), f"ldx > n, k={k}")
    assert_the_mix(list(it), f"ldx > n, k={k}")


# ------------------------------------------------------------------ the solves are the composition of the tested kernels
COMPOSED_M = (1, 2, 3, 4, 5, 11)
NEVER = 1e-150                        # rtol: thr = rtol^2 = 1e-300, nothing stops before max_iter


def device(E, values):
    return E.DeviceBuffer(len(values)).upload(values)


def composed_cg(E, s, b, inv_diag, L):
    """m -> (x, m, relative residual) for m in COMPOSED_M: ehyb_pcg's loop written out with ehyb_spmv and the step entry points"""
    lib, n, plan = E.host._lib.load(), s.n, s.plan
    d = {k: device(E, np.full(n, SENTINEL)) for k in ("r", "p", "q")}
    d["b"], d["x"], d["slots"] = device(E, b), device(E, np.zeros(n)), device(E, np.full(L["slots"] * MAX_GRID, SENTINEL))
    keep = device(E, inv_diag) if inv_diag is not None else None
    dinv = C.c_void_p(keep.ptr) if keep is not None else None
    P = {k: C.c_void_p(v.ptr) for k, v in d.items()}
    plan.spmv(d["x"].ptr, d["q"].ptr)
    assert lib.ehyb_cg_init_step(n, P["b"], P["q"], dinv, P["r"], P["p"], P["slots"], None) == 0
    out = {}
    for it in range(max(COMPOSED_M)):
        cur = it & 1
        plan.spmv(d["p"].ptr, d["q"].ptr)
        assert lib.ehyb_cg_dot_step(n, P["p"], P["q"], P["slots"], None) == 0
        assert lib.ehyb_cg_update_step(n, P["p"], P["q"], dinv, P["x"], P["r"], P["slots"], cur, None) == 0
        assert lib.ehyb_cg_direction_step(n, P["r"], dinv, P["p"], P["slots"], cur, None) == 0
        if it + 1 in COMPOSED_M:
            assert lib.ehyb_dev_sync() == 0
            sl = d["slots"].download().reshape(L["slots"], MAX_GRID)
            bb = sc.in_order_sum(sl[L["bb"]])
            out[it + 1] = (d["x"].download(), it + 1, math.sqrt(sc.in_order_sum(sl[L["rr"]]) / (bb if bb > 0 else 1.0)))
    return out


def composed_bicgstab(E, s, b, inv_diag, L):
    lib, n, plan = E.host._lib.load(), s.n, s.plan
    d = {k: device(E, np.full(n, SENTINEL)) for k in ("r", "rh", "p", "v", "sv", "sh", "t")}
    slots = np.full(L["slots"] * MAX_GRID + 1, SENTINEL)
    slots[-1] = np.zeros(2, dtype=np.int32).view(np.float64)[0]            # the solve zeroes the flags
    d["b"], d["x"], d["slots"] = device(E, b), device(E, np.zeros(n)), device(E, slots)
    keep = device(E, inv_diag) if inv_diag is not None else None
    dinv = C.c_void_p(keep.ptr) if keep is not None else None
    P = {k: C.c_void_p(v.ptr) for k, v in d.items()}
    thr = NEVER * NEVER
    plan.spmv(d["x"].ptr, d["v"].ptr, walk=1)
    assert lib.ehyb_bicgstab_init_step(n, P["b"], P["v"], dinv, P["r"], P["rh"], P["p"], P["slots"], None) == 0
    out = {}
    for it in range(max(COMPOSED_M)):
        cur = it & 1
        plan.spmv(d["p"].ptr, d["v"].ptr, walk=0)
        assert lib.ehyb_bicgstab_dot_step(n, P["rh"], P["v"], P["slots"], None) == 0
        assert lib.ehyb_bicgstab_s_step(n, P["r"], P["v"], dinv, P["sv"], P["sh"], P["slots"], cur, None) == 0
        plan.spmv(d["sh"].ptr, d["t"].ptr, walk=1)
        assert lib.ehyb_bicgstab_dot2_step(n, P["t"], P["sv"], P["slots"], None) == 0
        assert lib.ehyb_bicgstab_update_step(n, P["p"], P["sh"], P["sv"], P["t"], P["rh"], P["x"], P["r"], P["slots"], cur, thr, None) == 0
        assert lib.ehyb_bicgstab_direction_step(n, P["r"], P["v"], dinv, P["p"], P["slots"], cur, thr, None) == 0
        if it + 1 in COMPOSED_M:
            assert lib.ehyb_dev_sync() == 0
            raw = d["slots"].download()
            status, iters = (int(v) for v in raw[-1:].view(np.int32)[[L["flag_status"], L["flag_iters"]]])
            assert status == RUNNING
            sl = raw[:-1].reshape(L["slots"], MAX_GRID)
            bb = sc.in_order_sum(sl[L["slot_bb"]])
            out[it + 1] = (d["x"].download(), iters, math.sqrt(sc.in_order_sum(sl[L["slot_rr"]]) / (bb if bb > 0 else 1.0)))
    return out


def assert_solve_same_bits(got, want, what):
    x, it, rel = got
    xw, itw, relw = want
    assert it == itw, (what, it, itw)
    assert np.array_equal(np.array([rel]).view(np.int64), np.array([relw]).view(np.int64)), (what, rel, relw)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_pcg_is_the_composition_of_its_kernels(E, gpu, big_spd, cg_layout, jacobi):
    s = big_spd
    b = s.B[2]                                   # the random right-hand side
    inv = s.inv_diag if jacobi else None
    want = composed_cg(E, s, b, inv, cg_layout)
    for m in COMPOSED_M:
        assert want[m][1] == m
        for name, plan in (("graph replay", s.plan), ("graphs=2", s.plain_launches)):
            for check_every in (1, 4):
                got = plan.cg(b, max_iter=m, rtol=NEVER, check_every=check_every, inv_diag=inv)
                assert_solve_same_bits(got, want[m], f"ehyb_pcg m={m} {name} check_every={check_every} jacobi={jacobi}")


@pytest.fixture(scope="module")
def big_unsymmetric(E, gpu):
    return BigSystem(E, cd_matrix(FULL_NX, FULL_NY, 3000, 6), False, window_mode=2, lds_doubles=2048, sym_pairs=0)


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_bicgstab_is_the_composition_of_its_kernels(E, gpu, big_unsymmetric, bi_layout, jacobi):
    s = big_unsymmetric
    b = E.vector_reorder(np.random.default_rng(8).uniform(-1, 1, s.n), s.perm)
    inv = s.inv_diag if jacobi else None
    want = composed_bicgstab(E, s, b, inv, bi_layout)
    for m in COMPOSED_M:
        assert want[m][1] == m
        for name, plan in (("graph replay", s.plan), ("graphs=2", s.plain_launches)):
            for check_every in (1, 4):
                got = plan.bicgstab(b, max_iter=m, rtol=NEVER, check_every=check_every, inv_diag=inv)
                assert_solve_same_bits(got, want[m], f"ehyb_bicgstab m={m} {name} check_every={check_every} jacobi={jacobi}")
