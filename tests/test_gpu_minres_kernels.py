"""The four vector kernels of ehyb_minres one launch at a time through ehyb_minres_*_step, bit for bit, on the inputs of
minres_cases.py: every output is one number in fp64, so every vector, every single partial and every state double is compared
exactly (up to the sign of zero), at the sizes of solver_cases.SIZES -- every profile of unrolled and tail trips of the index
walk.  No tolerance appears in this file.

Guards of every step test, as in test_gpu_solver_kernels.py: each device vector has a pad of PAD doubles behind n that must keep
its sentinel; so must the outputs a kernel does not write, every slot it does not name, entries 512..1023 of the slots it
writes, the state copy it does not write and the pad behind the tail; entries 512..1023 of the slots a kernel READS hold NaN;
inputs come back unchanged.

The kernels at K = 2..4 have no step entry point: test_gpu_minres.py compares them with K = 1 column by column through the
solves, at a size past the unrolled loops too."""
import ctypes as C

import numpy as np
import pytest

import minres_cases as mc
import solver_cases as sc
from solver_cases import MAX_GRID, PAD, S, SENTINEL, STEP_GRID
from test_gpu_solver_kernels import assert_same, special_slot

pytestmark = pytest.mark.gpu

THR = 0.5625                  # rtol^2 of the step tests; with phibar = 3/2 and b.M^-1 b = 4 planted, phibar^2 == thr * bb exactly
RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2
HUGE, TINY = 2.0 ** 1000, 2.0 ** -1000


@pytest.fixture(scope="module")
def layout(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.MinresSlots()
    assert _lib.load().ehyb_minres_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert out["slot_doubles"] == MAX_GRID and (out["status_running"], out["status_converged"], out["status_breakdown"]) == (RUNNING, CONVERGED, BREAKDOWN)
    return out


class Bench:
    """The device side of one step test: named vectors of n doubles with a sentinel pad, the slot array with the tail (two
    state copies and the flags) and a pad behind it, one launch, and the comparison of EVERYTHING with what is expected."""

    def __init__(self, E, L, n, flags=(RUNNING, 41)):
        self.E, self.L, self.n, self.lib = E, L, n, E.host._lib.load()
        self.host, self.dev = {}, {}
        self.tail_at = L["slots"] * MAX_GRID
        self.s = np.full(self.tail_at + L["tail_doubles"] + PAD, SENTINEL)
        self.set_flags(*flags)

    def vec(self, name, values=None):
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

    def plant(self, which, fraction, seed=0):
        total, e = mc.planted_total(fraction)
        return self.slot(which, sc.planted_slot(total, e=e, seed=seed))

    def state(self, copy, values):
        for name, v in values.items():
            self.s[self.tail_at + copy * self.L["state_doubles"] + self.L["state_" + name]] = v
        return self

    def set_flags(self, status, iters):
        f = np.zeros(2, dtype=np.int32)
        f[self.L["flag_status"]], f[self.L["flag_iters"]] = status, iters
        self.s[self.tail_at + self.L["flags_at"]] = f.view(np.float64)[0]

    def call(self, fn, *args):
        """fn(n, ...) with names turned into device pointers ("slots": the slot array), None and numbers as they are"""
        if "slots" not in self.dev:
            self.dev["slots"] = self.E.DeviceBuffer(len(self.s)).upload(self.s)
            self.host["slots"] = self.s.copy()
        conv = [C.c_void_p(self.dev[a].ptr) if isinstance(a, str) else a for a in args]
        rc = getattr(self.lib, fn)(self.n, *conv, None)
        assert rc == 0, (fn, rc, self.lib.ehyb_last_error())
        assert self.lib.ehyb_dev_sync() == 0, (fn, self.lib.ehyb_last_error())

    def expect(self, what, vectors=(), slots=(), state=None, flags=None):
        """Everything on the device against the uploaded state, but for: vectors name -> new values of [0, n), slots which ->
        the first STEP_GRID entries, state (copy, name -> value), flags (status, iters).  The expected state becomes the new
        baseline."""
        L, h = self.L, self.host["slots"]
        for name, new in dict(vectors).items():
            self.host[name][:self.n] = new.f(name) if isinstance(new, sc.Fx) else new
        for which, new in dict(slots).items():
            h[which * MAX_GRID:which * MAX_GRID + STEP_GRID] = new.f(f"slot {which}") if isinstance(new, sc.Fx) else new
        if state is not None:
            copy, values = state
            for name, v in values.items():
                h[self.tail_at + copy * L["state_doubles"] + L["state_" + name]] = v
        if flags is not None:
            f = np.zeros(2, dtype=np.int32)
            f[L["flag_status"]], f[L["flag_iters"]] = flags
            h[self.tail_at + L["flags_at"]] = f.view(np.float64)[0]
        for name, want in self.host.items():
            got = self.dev[name].download()
            if name == "slots":
                for k in range(L["slots"]):
                    assert_same(got[k * MAX_GRID:(k + 1) * MAX_GRID], want[k * MAX_GRID:(k + 1) * MAX_GRID], f"{what}: slot {k}")
                assert_same(got[self.tail_at:self.tail_at + L["flags_at"]], want[self.tail_at:self.tail_at + L["flags_at"]], f"{what}: the state copies")
                fa = self.tail_at + L["flags_at"]
                assert tuple(got[fa:fa + 1].view(np.int32)) == tuple(want[fa:fa + 1].view(np.int32)), (what, "flags", got[fa:fa + 1].view(np.int32))
                assert np.array_equal(got[fa + 1:].view(np.int64), want[fa + 1:].view(np.int64)), f"{what}: the pad behind the tail"
            else:
                assert_same(got[:self.n], want[:self.n], f"{what}: {name}")
                assert np.array_equal(got[self.n:].view(np.int64), want[self.n:].view(np.int64)), f"{what}: the pad behind {name}"


def beta_slot(L, c):
    return L["slot_beta0"] + c


def variants():
    return [(cur, d) for cur in (0, 1) for d in (False, True)]


# ------------------------------------------------------------------ values, at every size
@pytest.mark.parametrize("n", sc.SIZES)
def test_init_step(E, gpu, layout, n):
    sc.asserted_walk(n)
    L = layout
    for with_dinv in (False, True):
        c = mc.minres_init_case(n, with_dinv, seed=n % 97)
        b = Bench(E, L, n).vecs(c["in"]).vec("r").vec("z")
        if with_dinv:
            b.vec("dinv", c["dinv"])
        b.call("ehyb_minres_init_step", "b", "q", "dinv" if with_dinv else None, "r", "z", "slots")
        b.expect(f"init n={n} inv_diag={with_dinv}", c["out"], {beta_slot(L, 0): c["sums"]["beta2"], L["slot_bb"]: c["sums"]["bb"]})


def dot_bench(E, L, n, cur, phibar, seed, bb=4):
    c = mc.minres_dot_case(n, seed=seed)
    b = Bench(E, L, n).vecs(c["in"]).slot(L["slot_bb"], sc.planted_slot(bb, seed=6))
    b.state(cur, dict(dbar=1.0, eps=2.0, phibar=phibar, cs=0.5, sn=0.25, beta_old=7.0))
    return c, b


@pytest.mark.parametrize("n", sc.SIZES)
def test_dot_step(E, gpu, layout, n):
    """phibar^2 = 9 > thr bb = 9/4: the partials of z.q.  The other state copy holds sentinels: it is not looked at."""
    sc.asserted_walk(n)
    for cur in (0, 1):
        c, b = dot_bench(E, layout, n, cur, 3.0, n % 89 + cur)
        b.call("ehyb_minres_dot_step", "z", "q", "slots", cur, THR)
        b.expect(f"dot n={n} cur={cur}", {}, {layout["slot_zq"]: c["sums"]["zq"]})


def lanczos_bench(E, L, n, cur, with_dinv, first, seed):
    c = mc.minres_lanczos_case(n, cur, with_dinv, first, seed=seed)
    sv = c["scalars"]
    b = Bench(E, L, n).vecs(c["in"]).vec("z")
    if first:
        b.vec("rb")
    if with_dinv:
        b.vec("dinv", c["dinv"])
    b.plant(beta_slot(L, cur), sv["beta2"], 1).plant(L["slot_zq"], sv["zq"], 2)
    b.slot(beta_slot(L, cur ^ 1), sc.planted_slot(11, seed=9, rest=SENTINEL))        # beta_old^2's slot: written, never read
    b.state(cur, dict(dbar=1.0, eps=2.0, phibar=3.0, cs=0.5, sn=0.25, beta_old=0.0 if first else float(sv["beta_old"])))
    return c, b


LANCZOS_ARGS = ("q", "ra", "rb", "dinv", "z", "slots")


def lanczos_args(with_dinv, cur):
    return tuple(a if a != "dinv" or with_dinv else None for a in LANCZOS_ARGS) + (cur,)


@pytest.mark.parametrize("first", [False, True], ids=["later", "first"])
@pytest.mark.parametrize("n", sc.SIZES)
def test_lanczos_step(E, gpu, layout, n, first):
    sc.asserted_walk(n)
    L = layout
    for cur, with_dinv in variants():
        c, b = lanczos_bench(E, L, n, cur, with_dinv, first, n % 83 + cur)
        b.call("ehyb_minres_lanczos_step", *lanczos_args(with_dinv, cur))
        b.expect(f"lanczos n={n} cur={cur} inv_diag={with_dinv} first={first}", c["out"], {beta_slot(L, cur ^ 1): c["sums"]["beta2_new"]})


def update_bench(E, L, n, cur, with_dinv, kind, seed, iters=41):
    c = mc.minres_update_case(n, cur, with_dinv, kind, seed=seed)
    sv = c["scalars"]
    b = Bench(E, L, n, flags=(RUNNING, iters)).vecs(c["in"])
    if with_dinv:
        b.vec("dinv", c["dinv"])
    b.plant(beta_slot(L, cur), sv["beta2"], 1).plant(L["slot_zq"], sv["zq"], 2).plant(beta_slot(L, cur ^ 1), sv["beta2_new"], 3)
    b.slot(L["slot_bb"], sc.planted_slot(4, seed=6))
    b.state(cur, sv["state"])
    return c, b


UPDATE_ARGS = ("ra", "dinv", "wa", "wb", "x", "slots")


def update_args(with_dinv, cur):
    return tuple(a if a != "dinv" or with_dinv else None for a in UPDATE_ARGS) + (cur,)


@pytest.mark.parametrize("kind", ["last", "triple"])
@pytest.mark.parametrize("n", sc.SIZES)
def test_update_step(E, gpu, layout, n, kind):
    """the rotation, w_new over wb, x += phi w_new, state copy cur ^ 1, counter + 1; the status stays.  After the "last" update
    phibar' = 0: the dot kernel of the next iteration (parity cur ^ 1) sets "converged" and writes nothing else."""
    sc.asserted_walk(n)
    L = layout
    for cur, with_dinv in variants():
        c, b = update_bench(E, L, n, cur, with_dinv, kind, n % 83 + cur)
        b.call("ehyb_minres_update_step", *update_args(with_dinv, cur))
        b.expect(f"update n={n} cur={cur} inv_diag={with_dinv} {kind}", c["out"], state=(cur ^ 1, c["scalars"]["state_new"]), flags=(RUNNING, 42))
        if kind == "last":
            b.vec("z", np.full(n, 3.0)).vec("q", np.full(n, 5.0))
            b.call("ehyb_minres_dot_step", "z", "q", "slots", cur ^ 1, 0.0)
            b.expect(f"dot after the last update n={n} cur={cur}", flags=(CONVERGED, 42))


def test_cur_is_masked(E, gpu, layout):
    L, n = layout, 3 * S + 1
    for passed in (2, 3):
        cur = passed & 1
        c, b = lanczos_bench(E, L, n, cur, True, False, 5)
        b.call("ehyb_minres_lanczos_step", *lanczos_args(True, passed))
        b.expect(f"lanczos cur={passed}", c["out"], {beta_slot(L, cur ^ 1): c["sums"]["beta2_new"]})
        c, b = update_bench(E, L, n, cur, True, "triple", 6)
        b.call("ehyb_minres_update_step", *update_args(True, passed))
        b.expect(f"update cur={passed}", c["out"], state=(cur ^ 1, c["scalars"]["state_new"]), flags=(RUNNING, 42))
        c, b = dot_bench(E, L, n, cur, 3.0, 7)
        b.call("ehyb_minres_dot_step", "z", "q", "slots", passed, THR)
        b.expect(f"dot cur={passed}", {}, {L["slot_zq"]: c["sums"]["zq"]})


# ------------------------------------------------------------------ the stop test
@pytest.mark.parametrize("n", [257, 4 * S + 1])
def test_dot_sets_converged_and_writes_nothing_else(E, gpu, layout, n):
    """phibar^2 == thr bb exactly (3/2, 4 and 9/16; and 3/4 against a planted b.b = 0, which counts as 1) is converged, one ulp
    more is not; the convergence test does not look at z.q, the beta^2 slots or the rest of the state (NaN there)."""
    L = layout
    for cur in (0, 1):
        for phibar, bb in ((1.5, 4), (0.75, 0), (-1.5, 4), (0.0, 4)):
            c, b = dot_bench(E, L, n, cur, phibar, 3, bb=bb)
            b.slot(L["slot_zq"], special_slot(np.nan)).slot(beta_slot(L, cur), special_slot(np.nan))
            b.state(cur, dict(dbar=np.nan, cs=np.nan, beta_old=np.nan))
            b.call("ehyb_minres_dot_step", "z", "q", "slots", cur, THR)
            b.expect(f"dot converged n={n} cur={cur} phibar={phibar}", flags=(CONVERGED, 41))
        c, b = dot_bench(E, L, n, cur, 1.5 * (1 + 2.0 ** -52), 3)
        b.call("ehyb_minres_dot_step", "z", "q", "slots", cur, THR)
        b.expect(f"dot one ulp above n={n} cur={cur}", {}, {L["slot_zq"]: c["sums"]["zq"]})


# ------------------------------------------------------------------ status behaviour
ALL_VECTORS = ("q", "ra", "rb", "z", "wa", "wb", "x", "dinv")


def healthy_state(E, L, n, cur, status=RUNNING, seed=0):
    """Every vector, every slot and the state of an iteration in flight, such that each of the three flagged steps would run to
    its end and write (the value tests above show that they do): phibar^2 = 9 against thr bb = 9/4, finite non-zero scalars."""
    rng = np.random.default_rng(seed)
    b = Bench(E, L, n, flags=(status, 41))
    for name in ALL_VECTORS:
        b.vec(name, rng.integers(1, 9, n).astype(np.float64) if name != "dinv" else np.full(n, 0.5))
    sv = mc.rotation_of(cur, "triple")
    b.plant(beta_slot(L, cur), sv["beta2"], 1).plant(L["slot_zq"], sv["zq"], 2).plant(beta_slot(L, cur ^ 1), sv["beta2_new"], 3)
    b.slot(L["slot_bb"], sc.planted_slot(4, seed=6))
    b.state(cur, dict(sv["state"], phibar=3.0, beta_old=float(sv["beta_old"])))
    return b


def launch_step(b, step, cur):
    args = {"dot": ("z", "q", "slots", cur, THR), "lanczos": LANCZOS_ARGS + (cur,), "update": UPDATE_ARGS + (cur,)}[step]
    b.call(f"ehyb_minres_{step}_step", *args)


FLAGGED_STEPS = ("dot", "lanczos", "update")
# (step, what is planted: "zq", "cur" / "new" (the beta^2 slot of parity cur / the other) -> the value of its sum, or a state
# double by name).  Each must end in breakdown.
BREAKDOWNS = [
    ("lanczos", {"zq": np.inf}), ("lanczos", {"zq": np.nan}), ("lanczos", {"cur": 0.0}), ("lanczos", {"cur": -4.0}),
    ("lanczos", {"cur": np.inf}), ("lanczos", {"cur": np.nan}), ("lanczos", {"zq": HUGE, "cur": TINY}), ("lanczos", {"beta_old": np.nan}),
    ("lanczos", {"beta_old": TINY, "cur": HUGE}),
    ("update", {"zq": np.inf}), ("update", {"zq": np.nan}), ("update", {"cur": 0.0}), ("update", {"cur": -4.0}), ("update", {"cur": np.nan}),
    ("update", {"new": -4.0}), ("update", {"new": np.inf}), ("update", {"new": np.nan}),
    ("update", {"new": 0.0, "dbar": 0.0, "cs": 0.0}),                 # gbar = 0 and beta_new = 0: gamma = 0
    ("update", {"dbar": HUGE}),                                        # gbar^2 overflows: gamma = inf
    ("update", {"dbar": np.nan}), ("update", {"phibar": np.inf}),
]


@pytest.mark.parametrize("case", range(len(BREAKDOWNS)), ids=[f"{s}-" + "-".join(f"{k}={v}" for k, v in p.items()) for s, p in BREAKDOWNS])
def test_breakdown_writes_the_status_and_nothing_else(E, gpu, layout, case):
    L, n = layout, 3 * S + 1
    step, plantings = BREAKDOWNS[case]
    cur = case & 1
    b = healthy_state(E, L, n, cur, seed=case)
    for name, value in plantings.items():
        if name in ("zq", "cur", "new"):
            b.slot({"zq": L["slot_zq"], "cur": beta_slot(L, cur), "new": beta_slot(L, cur ^ 1)}[name], special_slot(value))
        else:
            b.state(cur, {name: value})
    launch_step(b, step, cur)
    b.expect(f"{step} with {plantings}", flags=(BREAKDOWN, 41))
    for later in FLAGGED_STEPS:
        launch_step(b, later, cur)
        b.expect(f"{later} after the breakdown in {step}", flags=(BREAKDOWN, 41))


def test_a_zero_beta_new_alone_is_no_breakdown(E, gpu, layout):
    """beta_new = 0 with gamma = |gbar| > 0 is the last update (test_update_step, kind "last"); here on the healthy state:
    the update runs, the counter advances, the status stays"""
    L, n = layout, 257
    for cur in (0, 1):
        b = healthy_state(E, L, n, cur).slot(beta_slot(L, cur ^ 1), special_slot(0.0))
        launch_step(b, "update", cur)
        assert b.dev["slots"].download()[b.tail_at + L["flags_at"]:][:1].view(np.int32).tolist() == [RUNNING, 42]


@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
def test_steps_return_at_once_when_the_status_is_set(E, gpu, layout, status):
    L = layout
    for n in (257, 4 * S + 1):
        for cur in (0, 1):
            b = healthy_state(E, L, n, cur, status=status, seed=n % 5)
            for step in FLAGGED_STEPS:
                launch_step(b, step, cur)
                b.expect(f"{step} with the status preset to {status}, n={n}", flags=(status, 41))


@pytest.mark.parametrize("probe", sc.DIVISION_PROBES, ids=[f"probe{i}" for i in range(len(sc.DIVISION_PROBES))])
def test_the_lanczos_scalars_are_correctly_rounded(E, gpu, layout, probe):
    """beta / beta_old = 1 / P (beta^2 = 1 planted, beta_old = P in the state) read back as r_new[0] = fma(-(beta / beta_old), -1, 0);
    and, for P > 0, alpha / beta with alpha = R / P and beta = sqrt(P) -- a division, a root and a division, each rounded once --
    read back the same way in the first-iteration form."""
    L, n, (R, P) = layout, 257, probe
    first = np.zeros(n)
    first[0] = 1.0
    zero = np.zeros(n)
    # later form, q = 0, ra = 0, rb = -e_0: r_new[0] = beta / beta_old = 1 / P, correctly rounded
    b = Bench(E, L, n).vecs({"q": zero, "ra": zero, "rb": -first}).vec("z")
    b.slot(beta_slot(L, 0), sc.planted_slot(1, seed=1)).slot(L["slot_zq"], sc.planted_slot(R, seed=2))
    b.state(0, dict(dbar=1.0, eps=2.0, phibar=3.0, cs=0.5, sn=0.25, beta_old=float(P)))
    b.call("ehyb_minres_lanczos_step", "q", "ra", "rb", None, "z", "slots", 0)
    want = first * (1.0 / float(P))
    b2 = np.zeros(STEP_GRID)
    b2[0] = want[0] * want[0]               # one non-zero term, fma(r, r, 0): one rounding, the same fused or not
    b.expect(f"beta / beta_old = 1 / {P}", {"rb": want, "z": want}, {beta_slot(L, 1): b2})
    # first form, q = 0, ra = -e_0, beta^2 = P: r_new[0] = alpha / beta
    b = Bench(E, L, n).vecs({"q": zero, "ra": -first}).vec("rb").vec("z")
    b.slot(beta_slot(L, 0), sc.planted_slot(P, seed=1)).slot(L["slot_zq"], sc.planted_slot(R, seed=2))
    b.state(0, dict(dbar=1.0, eps=2.0, phibar=3.0, cs=0.5, sn=0.25, beta_old=0.0))
    if P > 0:
        alpha = sc.rounded_quotient(R, P)
        beta = float(np.sqrt(np.float64(P)))
        want = first * (alpha / beta)
        b2[0] = want[0] * want[0]
        b.call("ehyb_minres_lanczos_step", "q", "ra", "rb", None, "z", "slots", 0)
        b.expect(f"alpha / beta from {R} / {P}", {"rb": want, "z": want}, {beta_slot(L, 1): b2})
