"""The six vector kernels of ehyb_lsqr one launch at a time through ehyb_lsqr_*_step, on K = 1 .. 4 columns, on the inputs of
lsqr_cases.py: every vector, every single partial and every state double is ONE number in fp64 and is compared exactly (up to the
sign of zero), at sizes that cover the profiles of unrolled and tail trips of the index walk.  The one exception is named where
it is made: the four state doubles behind gamma = hypot(gbar, theta), whose last bit is the math library's (LOOSE, 4 ulp).

Guards of every step test, as in test_gpu_minres_kernels.py: each device vector has a pad of PAD doubles behind k * n that must
keep its sentinel; so must the columns and outputs a kernel does not write, every slot it does not name, entries 512..1023 of the
slots it writes, the state copy it does not write and the pad behind the tails; entries 512..1023 of the slots a kernel READS
hold NaN; inputs come back unchanged.  From K = 2 on column 1 has its status set: every flagged step must leave it alone while
it serves the others."""
import ctypes as C

import numpy as np
import pytest

import lsqr_cases as lc
import solver_cases as sc
from solver_cases import MAX_GRID, PAD, S, SENTINEL, STEP_GRID
from test_gpu_solver_kernels import assert_same, special_slot

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2
SIZES = [0, 1, 63, 64, 65, 257, S - 1, S + 1, 2 * S + 77, 4 * S + 1]
KS = [1, 2, 3, 4]
NEVER = 1e-150                           # atol = btol of the step tests that must not stop
LOOSE = ("cs2", "sn2", "z", "xxnorm")    # the state doubles behind gamma = hypot(gbar, theta)
BIG2, TINY2 = 2.0 ** 1020, 2.0 ** -1060   # squares whose roots are finite and whose ratio of roots, 2^1040, is not
# a state copy on which neither stop test holds
GOING = dict(rhobar=1.0, phibar=1.0, cs2=-1.0, sn2=0.0, z=0.0, xxnorm=0.0, res2=0.0, anorm2=4.0, rnorm=3.0, arnorm=5.0, xnorm=2.0, bnorm=1.0)


@pytest.fixture(scope="module")
def layout(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.LsqrSlots()
    assert _lib.load().ehyb_lsqr_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert out["slot_doubles"] == MAX_GRID and (out["status_running"], out["status_converged"], out["status_breakdown"]) == (RUNNING, CONVERGED, BREAKDOWN)
    return out


def statuses(k, preset=CONVERGED):
    """column 1 of a launch of two or more has its status set"""
    return [preset if (c == 1 and k >= 2) else RUNNING for c in range(k)]


class Bench:
    """The device side of one step test on k columns: named vectors of k * n doubles with a sentinel pad, the slot array with the
    k tails and a pad behind them, one launch, and the comparison of EVERYTHING with what is expected."""

    def __init__(self, E, L, n, k, status=None, iters=41):
        self.E, self.L, self.n, self.k, self.lib = E, L, n, k, E.host._lib.load()
        self.host, self.dev = {}, {}
        self.tail_at = k * L["slots"] * MAX_GRID
        self.s = np.full(self.tail_at + k * L["tail_doubles"] + PAD, SENTINEL)
        for c in range(k):
            self.set_flags(self.s, c, (status or [RUNNING] * k)[c], iters)

    def _values(self, v, name):
        return v.f(name) if isinstance(v, sc.Fx) else v

    def vec(self, name, columns=None):
        """columns: per column an Fx or an array of n values (None: the sentinel, an output)"""
        h = np.full(self.k * self.n + PAD, SENTINEL)
        for c, v in enumerate(columns or []):
            if v is not None:
                h[c * self.n:(c + 1) * self.n] = self._values(v, name)
        self.host[name] = h
        self.dev[name] = self.E.DeviceBuffer(len(h)).upload(h)
        return self

    def slot_at(self, c, which):
        return (c * self.L["slots"] + which) * MAX_GRID

    def slot(self, c, which, values):
        self.s[self.slot_at(c, which):self.slot_at(c, which) + MAX_GRID] = values
        return self

    def plant(self, c, which, fraction, seed=0):
        total, e = lc.planted_total(fraction)
        return self.slot(c, which, sc.planted_slot(total, e=e, seed=seed + 10 * c))

    def state_at(self, c, copy, name):
        return self.tail_at + c * self.L["tail_doubles"] + copy * self.L["state_doubles"] + self.L["state_" + name]

    def state(self, c, copy, values):
        for name, v in values.items():
            self.s[self.state_at(c, copy, name)] = v
        return self

    def set_flags(self, s, c, status, iters):
        f = np.zeros(2, dtype=np.int32)
        f[self.L["flag_status"]], f[self.L["flag_iters"]] = status, iters
        s[self.tail_at + c * self.L["tail_doubles"] + self.L["flags_at"]] = f.view(np.float64)[0]

    def call(self, fn, *args):
        """fn(n, k, ...) with names turned into device pointers ("slots": the slot array), numbers as they are"""
        if "slots" not in self.dev:
            self.dev["slots"] = self.E.DeviceBuffer(len(self.s)).upload(self.s)
            self.host["slots"] = self.s.copy()
        conv = [C.c_void_p(self.dev[a].ptr) if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, fn)(self.n, self.k, *conv, None)
        assert rc == 0, (fn, rc, self.lib.ehyb_last_error())
        assert self.lib.ehyb_dev_sync() == 0, (fn, self.lib.ehyb_last_error())

    def expect(self, what, vectors=(), slots=(), state=(), flags=(), loose=()):
        """Everything on the device against the uploaded state, but for: vectors (name, column) -> new values of the column, slots
        (column, which) -> the first STEP_GRID entries, state (column, copy) -> name -> value, flags column -> (status, iters),
        loose: (column, copy, name) compared within 4 ulp.  The expected state becomes the new baseline."""
        L, h, n = self.L, self.host["slots"], self.n
        for (name, c), new in dict(vectors).items():
            self.host[name][c * n:(c + 1) * n] = self._values(new, name)
        for (c, which), new in dict(slots).items():
            h[self.slot_at(c, which):self.slot_at(c, which) + STEP_GRID] = self._values(new, f"slot {which}")
        for (c, copy), values in dict(state).items():
            for name, v in values.items():
                h[self.state_at(c, copy, name)] = v
        for c, (status, iters) in dict(flags).items():
            self.set_flags(h, c, status, iters)
        for name, want in self.host.items():
            got = self.dev[name].download()
            if name != "slots":
                for c in range(self.k):
                    assert_same(got[c * n:(c + 1) * n], want[c * n:(c + 1) * n], f"{what}: {name}, column {c}")
                assert np.array_equal(got[self.k * n:].view(np.int64), want[self.k * n:].view(np.int64)), f"{what}: the pad behind {name}"
                continue
            for c, copy, field in loose:
                at = self.state_at(c, copy, field)
                assert abs(got[at] - want[at]) <= 4 * np.spacing(abs(want[at])), (what, c, field, got[at], want[at])
                want[at] = got[at]
            for c in range(self.k):
                for w in range(L["slots"]):
                    a = self.slot_at(c, w)
                    assert_same(got[a:a + MAX_GRID], want[a:a + MAX_GRID], f"{what}: column {c}, slot {w}")
                t = self.tail_at + c * L["tail_doubles"]
                assert_same(got[t:t + L["flags_at"]], want[t:t + L["flags_at"]], f"{what}: column {c}, the state copies")
                fa = t + L["flags_at"]
                assert tuple(got[fa:fa + 1].view(np.int32)) == tuple(want[fa:fa + 1].view(np.int32)), (what, c, "flags", got[fa:fa + 1].view(np.int32))
            end = self.tail_at + self.k * L["tail_doubles"]
            assert np.array_equal(got[end:].view(np.int64), want[end:].view(np.int64)), f"{what}: the pad behind the tails"


def sizes_and_widths(f):
    return pytest.mark.parametrize("k", KS)(pytest.mark.parametrize("n", SIZES)(f))


def columns(k, make):
    return [make(c) for c in range(k)]


# ------------------------------------------------------------------ init, start: no tail, every column is served
@sizes_and_widths
def test_init_step(E, gpu, layout, n, k):
    sc.asserted_walk(n)
    L = layout
    cs = columns(k, lambda c: lc.lsqr_init_case(n, seed=n % 97 + c))
    b = Bench(E, L, n, k).vec("b", [c["in"]["b"] for c in cs]).vec("t", [c["in"]["t"] for c in cs]).vec("u")
    b.call("ehyb_lsqr_init_step", "b", "t", "u", "slots")
    b.expect(f"init n={n} k={k}", {("u", c): cs[c]["out"]["u"] for c in range(k)},
             {**{(c, L["slot_beta0"]): cs[c]["sums"]["beta2"] for c in range(k)}, **{(c, L["slot_bb"]): cs[c]["sums"]["bb"] for c in range(k)}})


@sizes_and_widths
def test_start_step(E, gpu, layout, n, k):
    """V = t / beta_1 and the partials of alpha_1^2; from K = 2 on column 1 has beta_1^2 = 0 (b = A x0): nothing is written for it"""
    sc.asserted_walk(n)
    L = layout
    cs = columns(k, lambda c: lc.lsqr_start_case(n, c & 1, seed=n % 89 + c))
    off = [c == 1 and k >= 2 for c in range(k)]
    b = Bench(E, L, n, k).vec("t", [c["in"]["t"] for c in cs]).vec("v")
    for c in range(k):
        if off[c]:
            b.slot(c, L["slot_beta0"], special_slot(0.0))
        else:
            b.plant(c, L["slot_beta0"], cs[c]["beta2"], 1)
    b.call("ehyb_lsqr_start_step", "t", "v", "slots")
    b.expect(f"start n={n} k={k}", {("v", c): cs[c]["out"]["v"] for c in range(k) if not off[c]},
             {(c, L["slot_alpha0"]): cs[c]["sums"]["alpha2"] for c in range(k) if not off[c]})


@pytest.mark.parametrize("value", [np.nan, np.inf, -4.0])
def test_start_leaves_a_column_with_a_bad_beta_alone(E, gpu, layout, value):
    L, n = layout, 257
    c = lc.lsqr_start_case(n, 0)
    b = Bench(E, L, n, 1).vec("t", [c["in"]["t"]]).vec("v").slot(0, L["slot_beta0"], special_slot(value))
    b.call("ehyb_lsqr_start_step", "t", "v", "slots")
    b.expect(f"start with beta_1^2 = {value}")


# ------------------------------------------------------------------ the flagged steps, at every size and width
@sizes_and_widths
def test_wstart_step(E, gpu, layout, n, k):
    sc.asserted_walk(n)
    L = layout
    cs = columns(k, lambda c: lc.lsqr_wstart_case(n, c & 1, seed=n % 83 + c))
    st = statuses(k)
    b = Bench(E, L, n, k, status=st).vec("v", [c["in"]["v"] for c in cs]).vec("w")
    for c in range(k):
        b.plant(c, L["slot_alpha0"], cs[c]["alpha2"], 2)
    b.call("ehyb_lsqr_wstart_step", "v", "w", "slots")
    b.expect(f"wstart n={n} k={k}", {("w", c): cs[c]["out"]["w"] for c in range(k) if st[c] == RUNNING})


def pair_bench(E, L, n, k, cur, step, st=None, seed=0):
    """ustep (new = U, divisor alpha, ratio alpha / beta) or vstep (new = V, divisor beta', ratio beta' / alpha) on k columns;
    column c uses the scalars of parity (cur + c) & 1 of lsqr_cases.PAIR"""
    cs = columns(k, lambda c: lc.lsqr_pair_case(n, (cur + c) & 1, seed=seed + c))
    b = Bench(E, L, n, k, status=st).vec("t", [c["in"]["t"] for c in cs]).vec("old", [c["in"]["old"] for c in cs])
    for c in range(k):
        d2, e2 = cs[c]["d2"], cs[c]["e2"]
        if step == "ustep":                 # alpha^2 = d^2 and beta^2 = e^2 of parity cur; writes beta^2 of the other parity
            b.plant(c, L["slot_alpha0"] + cur, d2, 1).plant(c, L["slot_beta0"] + cur, e2, 2)
            b.slot(c, L["slot_beta0"] + (cur ^ 1), sc.planted_slot(11, seed=9, rest=SENTINEL))
        else:                               # beta'^2 = d^2 of parity cur ^ 1, alpha^2 = e^2 of parity cur; writes alpha^2 of cur ^ 1
            b.plant(c, L["slot_beta0"] + (cur ^ 1), d2, 1).plant(c, L["slot_alpha0"] + cur, e2, 2)
            b.slot(c, L["slot_alpha0"] + (cur ^ 1), sc.planted_slot(11, seed=9, rest=SENTINEL))
        b.state(c, cur, GOING)
    return cs, b


def launch_pair(b, step, cur):
    if step == "ustep":
        b.call("ehyb_lsqr_ustep_step", "t", "old", "slots", cur, NEVER, NEVER)
    else:
        b.call("ehyb_lsqr_vstep_step", "t", "old", "slots", cur)


def written_slot(L, step, cur):
    return (L["slot_beta0"] if step == "ustep" else L["slot_alpha0"]) + (cur ^ 1)


@pytest.mark.parametrize("step", ["ustep", "vstep"])
@sizes_and_widths
def test_ustep_and_vstep(E, gpu, layout, n, k, step):
    sc.asserted_walk(n)
    L = layout
    for cur in (0, 1):
        st = statuses(k, BREAKDOWN if cur else CONVERGED)
        cs, b = pair_bench(E, L, n, k, cur, step, st, seed=n % 79 + 7 * cur)
        launch_pair(b, step, cur)
        on = [c for c in range(k) if st[c] == RUNNING]
        b.expect(f"{step} n={n} k={k} cur={cur}", {("old", c): cs[c]["out"]["new"] for c in on},
                 {(c, written_slot(L, step, cur)): cs[c]["sums"]["new2"] for c in on})


def update_bench(E, L, n, k, cur, lucky, st=None, seed=0, iters=41):
    """every column uses the planted set `cur` of lsqr_cases.UPDATE (damp is an argument of the launch: the columns share it) on
    vectors of its own"""
    cs = columns(k, lambda c: lc.lsqr_update_case(n, cur, lucky, seed=seed + c))
    b = Bench(E, L, n, k, status=st, iters=iters)
    b.vec("v", [c["in"].get("v") for c in cs]).vec("w", [c["in"]["w"] for c in cs]).vec("x", [c["in"]["x"] for c in cs])
    for c in range(k):
        sv = cs[c]["scalars"]
        b.plant(c, L["slot_alpha0"] + cur, sv["alpha2"], 1).plant(c, L["slot_beta0"] + (cur ^ 1), sv["beta2_n"], 2)
        b.plant(c, L["slot_alpha0"] + (cur ^ 1), sv["alpha2_n"], 3)
        b.state(c, cur, sv["state"])
    return cs, b


@pytest.mark.parametrize("lucky", [None, "beta", "alpha"], ids=["both", "beta-zero", "alpha-zero"])
@sizes_and_widths
def test_update_step(E, gpu, layout, n, k, lucky):
    """the rotations, x and w, state copy cur ^ 1, counter + 1; the status stays.  beta' = 0: the alpha'^2 slot holds 7 and is not
    used, V (sentinels) is not read, w stays.  Afterwards arnorm = 0 where a scalar was zero: the ustep kernel of the next
    iteration sets "converged" by test 2 and writes nothing else."""
    sc.asserted_walk(n)
    L = layout
    for cur in (0, 1):
        st = statuses(k, CONVERGED if cur else BREAKDOWN)
        cs, b = update_bench(E, L, n, k, cur, lucky, st, seed=n % 73 + 5 * cur)
        b.call("ehyb_lsqr_update_step", "v", "w", "x", "slots", cur, cs[0]["scalars"]["damp"])
        on = [c for c in range(k) if st[c] == RUNNING]
        vectors = {(name, c): cs[c]["out"][name] for c in on for name in cs[c]["out"]}
        b.expect(f"update n={n} k={k} cur={cur} {lucky}", vectors, state={(c, cur ^ 1): cs[c]["scalars"]["state_new"] for c in on},
                 flags={c: (RUNNING, 42) for c in on}, loose=[(c, cur ^ 1, f) for c in on for f in LOOSE])
        if lucky and n in (257, 4 * S + 1):
            b.vec("t", [np.full(n, 3.0)] * k)
            b.call("ehyb_lsqr_ustep_step", "t", "w", "slots", cur ^ 1, 0.0, 0.0)
            b.expect(f"ustep after the lucky update n={n} cur={cur}", flags={c: (CONVERGED, 42) for c in on})


def test_cur_is_masked(E, gpu, layout):
    L, n, k = layout, 3 * S + 1, 2
    for passed in (2, 3):
        cur = passed & 1
        for step in ("ustep", "vstep"):
            cs, b = pair_bench(E, L, n, k, cur, step, seed=5)
            launch_pair(b, step, passed)
            b.expect(f"{step} cur={passed}", {("old", c): cs[c]["out"]["new"] for c in range(k)},
                     {(c, written_slot(L, step, cur)): cs[c]["sums"]["new2"] for c in range(k)})
        cs, b = update_bench(E, L, n, k, cur, None, seed=6)
        b.call("ehyb_lsqr_update_step", "v", "w", "x", "slots", passed, cs[0]["scalars"]["damp"])
        b.expect(f"update cur={passed}", {(name, c): cs[c]["out"][name] for c in range(k) for name in ("x", "w")},
                 state={(c, cur ^ 1): cs[c]["scalars"]["state_new"] for c in range(k)}, flags={c: (RUNNING, 42) for c in range(k)},
                 loose=[(c, cur ^ 1, f) for c in range(k) for f in LOOSE])


# ------------------------------------------------------------------ the stop tests
@pytest.mark.parametrize("n", [257, 4 * S + 1])
def test_ustep_sets_converged_and_writes_nothing_else(E, gpu, layout, n):
    """atol = 1/4, btol = 1/2 on anorm = 2, xnorm = 3, bnorm = 4: test 1 is rnorm <= 7/2, test 2 arnorm <= rnorm / 2.  Equality
    counts, one ulp more does not; the tests do not look at the slots or at the rest of the state (NaN there)."""
    L = layout
    base = dict(anorm2=4.0, xnorm=3.0, bnorm=4.0)
    up = 1 + 2.0 ** -52
    stops = [dict(rnorm=3.5, arnorm=9.0), dict(rnorm=0.0, arnorm=9.0), dict(rnorm=8.0, arnorm=4.0), dict(rnorm=8.0, arnorm=0.0)]
    goes = [dict(rnorm=3.5 * up, arnorm=3.5), dict(rnorm=8.0, arnorm=4.0 * up), dict(rnorm=np.nan, arnorm=1.0)]
    for cur in (0, 1):
        for values in stops:
            cs, b = pair_bench(E, L, n, 1, cur, "ustep", seed=3)
            b.slot(0, L["slot_alpha0"] + cur, special_slot(np.nan)).slot(0, L["slot_beta0"] + cur, special_slot(np.nan))
            b.state(0, cur, dict(dict.fromkeys(lc.STATE, np.nan), **base, **values))
            b.call("ehyb_lsqr_ustep_step", "t", "old", "slots", cur, 0.25, 0.5)
            b.expect(f"ustep converged n={n} cur={cur} {values}", flags={0: (CONVERGED, 41)})
        for values in goes:
            cs, b = pair_bench(E, L, n, 1, cur, "ustep", seed=3)
            b.state(0, cur, dict(dict.fromkeys(lc.STATE, np.nan), **base, **values))
            b.call("ehyb_lsqr_ustep_step", "t", "old", "slots", cur, 0.25, 0.5)
            b.expect(f"ustep goes on n={n} cur={cur} {values}", {("old", 0): cs[0]["out"]["new"]}, {(0, L["slot_beta0"] + (cur ^ 1)): cs[0]["sums"]["new2"]})


# ------------------------------------------------------------------ status behaviour
def healthy(E, L, n, k, cur, step, st=None, seed=0):
    if step == "update":
        return update_bench(E, L, n, k, cur, None, st, seed)[1]
    if step == "wstart":
        cs = columns(k, lambda c: lc.lsqr_wstart_case(n, c & 1, seed=seed + c))
        b = Bench(E, L, n, k, status=st).vec("v", [c["in"]["v"] for c in cs]).vec("w")
        for c in range(k):
            b.plant(c, L["slot_alpha0"], cs[c]["alpha2"], 2)
        return b
    return pair_bench(E, L, n, k, cur, step, st, seed)[1]


def launch(b, step, cur):
    if step == "update":
        b.call("ehyb_lsqr_update_step", "v", "w", "x", "slots", cur, float(lc.UPDATE[cur]["damp"]))
    elif step == "wstart":
        b.call("ehyb_lsqr_wstart_step", "v", "w", "slots")
    else:
        launch_pair(b, step, cur)


FLAGGED = ("wstart", "ustep", "vstep", "update")


@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
@pytest.mark.parametrize("k", KS)
def test_steps_return_at_once_when_every_status_is_set(E, gpu, layout, status, k):
    L = layout
    for n, cur in ((257, 0), (257, 1), (4 * S + 1, 1)):
        for step in FLAGGED:
            b = healthy(E, L, n, k, cur, step, st=[status] * k, seed=n % 5)
            launch(b, step, cur)
            b.expect(f"{step} with the status preset to {status}, n={n} k={k}")


# (step, what is planted: "a" / "b" = the alpha^2 / beta^2 slot of parity cur, "an" / "bn" = of the other parity -> the value of
# its sum, or a state double by name).  Each must end in breakdown.
BREAKDOWNS = [
    ("wstart", {"a0": 0.0}), ("wstart", {"a0": np.nan}), ("wstart", {"a0": np.inf}),
    ("ustep", {"a": 0.0}), ("ustep", {"a": np.nan}), ("ustep", {"a": np.inf}), ("ustep", {"a": -4.0}), ("ustep", {"b": 0.0}), ("ustep", {"b": np.nan}),
    ("ustep", {"b": np.inf}), ("ustep", {"a": BIG2, "b": TINY2}),
    ("vstep", {"a": 0.0}), ("vstep", {"a": np.nan}), ("vstep", {"bn": np.nan}), ("vstep", {"bn": np.inf}), ("vstep", {"bn": -4.0}),
    ("vstep", {"bn": BIG2, "a": TINY2}),
    ("update", {"bn": np.nan}), ("update", {"bn": np.inf}), ("update", {"an": np.nan}), ("update", {"an": np.inf}), ("update", {"bn": -1.0}),
    ("update", {"rhobar": 0.0, "bn": 0.0, "damp": 0.0}),           # rho = 0
    ("update", {"rhobar": np.nan}), ("update", {"rhobar": np.inf}),
    ("update", {"phibar": np.inf}), ("update", {"phibar": np.nan}),
]


@pytest.mark.parametrize("case", range(len(BREAKDOWNS)), ids=[f"{s}-" + "-".join(f"{k}={v}" for k, v in p.items()) for s, p in BREAKDOWNS])
def test_breakdown_writes_the_status_and_nothing_else(E, gpu, layout, case):
    """in column 0 of two: column 1 is served as if alone.  Then every flagged step leaves the broken column alone."""
    L, n, k = layout, 3 * S + 1, 2
    step, plantings = BREAKDOWNS[case]
    cur = case & 1
    b = healthy(E, L, n, k, cur, step, seed=case)
    damp = float(lc.UPDATE[cur]["damp"])
    for name, value in plantings.items():
        where = {"a0": L["slot_alpha0"], "a": L["slot_alpha0"] + cur, "b": L["slot_beta0"] + cur, "an": L["slot_alpha0"] + (cur ^ 1),
                 "bn": L["slot_beta0"] + (cur ^ 1)}
        if name in where:
            b.slot(0, where[name], special_slot(value))
        elif name == "damp":
            damp = value
        else:
            b.state(0, cur, {name: value})
    if step == "update":
        b.call("ehyb_lsqr_update_step", "v", "w", "x", "slots", cur, damp)
    else:
        launch(b, step, cur)
    got = b.dev["slots"].download()
    f0 = got[b.tail_at + L["flags_at"]:][:1].view(np.int32).tolist()
    assert f0 == [BREAKDOWN, 41], (step, plantings, f0)
    # everything of column 0 is as it was but the status; column 1's outputs are the launch's business, shown by the value tests
    for name in b.host:
        if name == "slots":
            continue
        assert_same(b.dev[name].download()[:n], b.host[name][:n], f"{step} with {plantings}: {name}, column 0")
    want = b.host["slots"]
    b.set_flags(want, 0, BREAKDOWN, 41)
    t = b.tail_at
    assert_same(got[:L["slots"] * MAX_GRID], want[:L["slots"] * MAX_GRID], "column 0's slots")
    assert_same(got[t:t + L["flags_at"]], want[t:t + L["flags_at"]], "column 0's state copies")


def test_a_zero_beta_new_alone_is_no_breakdown_and_vstep_skips(E, gpu, layout):
    """beta' = 0 with rho = rhobar1 > 0 is the lucky end (test_update_step, beta-zero); here the vstep kernel: nothing is
    written, the status stays"""
    L, n = layout, 257
    for cur in (0, 1):
        cs, b = pair_bench(E, L, n, 1, cur, "vstep", seed=2)
        b.slot(0, L["slot_beta0"] + (cur ^ 1), special_slot(0.0))
        launch_pair(b, "vstep", cur)
        b.expect(f"vstep with beta' = 0, cur={cur}")


@pytest.mark.parametrize("probe", sc.DIVISION_PROBES, ids=[f"probe{i}" for i in range(len(sc.DIVISION_PROBES))])
def test_the_pair_scalars_are_correctly_rounded(E, gpu, layout, probe):
    """alpha / beta with alpha^2 = |R|, beta^2 = |P| planted: two roots and a division, each rounded once, read back as
    U[0] = fma(-(alpha / beta), -1, 0 / alpha); and t / alpha as a true division: U[256] = 1 / alpha (in the next workgroup, so
    that each partial of beta'^2 is one rounded square)"""
    L, n, (R, P) = layout, 257, probe
    R, P = abs(R), abs(P)
    old, t = np.zeros(n), np.zeros(n)
    old[0], t[256] = -1.0, 1.0
    b = Bench(E, L, n, 1).vec("t", [t]).vec("old", [old])
    b.slot(0, L["slot_alpha0"], sc.planted_slot(R, seed=1)).slot(0, L["slot_beta0"], sc.planted_slot(P, seed=2)).state(0, 0, GOING)
    b.call("ehyb_lsqr_ustep_step", "t", "old", "slots", 0, NEVER, NEVER)
    alpha, beta = np.sqrt(np.float64(R)), np.sqrt(np.float64(P))
    want = np.zeros(n)
    want[0], want[256] = alpha / beta, 1.0 / alpha
    b2 = np.zeros(STEP_GRID)
    b2[0], b2[1] = want[0] * want[0], want[256] * want[256]
    b.expect(f"alpha / beta from {R}, {P}", {("old", 0): want}, {(0, L["slot_beta0"] + 1): b2})
