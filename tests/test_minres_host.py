"""ehyb_minres, ehyb_minres_multi, ehyb_minres_layout and the ehyb_minres_*_step building blocks on the host: every argument
check and their order on plans that were never uploaded, the consistency of the published layout, and the step entry points'
own checks -- all before any device work, so nothing here needs a GPU."""
import ctypes as C

import pytest

ERR_ARG, ERR_STATE = 1, 8                # EHYB_ERR_ARG, EHYB_ERR_STATE
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))


def host_plan(E, half=False, **kw):
    """half: a plan over the rows up to the middle partition boundary (the multi-GPU sharding) instead of every row"""
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(FEM_SMALL[0], *FEM_SMALL[1], cfg=cfg)
    m.reorder(cfg)
    pb = m.part_boundary
    return E.Plan(m, cfg, rows=(0, int(pb[len(pb) // 2])) if half else None, upload=False)


@pytest.fixture(scope="module")
def plan(E):
    return host_plan(E, direct=2)


@pytest.fixture(scope="module")
def part(E):
    p = host_plan(E, half=True, direct=2)
    assert 0 < p.rows[1] < p.n
    return p


B, X, D = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)   # never read: every call fails before device work


def call_one(lib, plan, h=None, d=D, b=B, x=X, max_iter=50, rtol=1e-8, check_every=10, outputs=True):
    it, rel = C.c_int(-5), C.c_double(-5.0)
    rc = lib.ehyb_minres(plan.h if h is None else h, d, b, x, max_iter, rtol, check_every, None, C.byref(it) if outputs else None,
                         C.byref(rel) if outputs else None)
    return rc, lib.ehyb_last_error()


def call_multi(lib, plan, d=D, b=B, ldb=None, x=X, ldx=None, k=3, max_iter=50, rtol=1e-8, check_every=10, outputs=True):
    n = plan.n
    it = (C.c_int * 16)() if outputs else None
    rel = (C.c_double * 16)() if outputs else None
    rc = lib.ehyb_minres_multi(plan.h, d, b, n if ldb is None else ldb, x, n if ldx is None else ldx, k, max_iter, rtol, check_every, None,
                               it, rel)
    return rc, lib.ehyb_last_error()


def says_one_vector(msg):
    return b"ehyb_minres:" in msg and b"_multi" not in msg


# ------------------------------------------------------------------ ehyb_minres
def test_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    rc, msg = call_one(lib, plan)
    assert rc == ERR_STATE and b"upload" in msg and says_one_vector(msg), msg
    # zero iterations, rtol = 0, check_every <= 0, no preconditioner, no outputs: still only the upload is missing
    for kw in (dict(max_iter=0), dict(rtol=0.0), dict(check_every=0), dict(check_every=-3), dict(d=None), dict(outputs=False),
               dict(d=None, outputs=False, max_iter=0, check_every=0)):
        rc, msg = call_one(lib, plan, **kw)
        assert rc == ERR_STATE and says_one_vector(msg), (kw, msg)


BAD = [dict(b=None), dict(x=None), dict(max_iter=-1), dict(rtol=-1e-9), dict(rtol=float("nan")), dict(rtol=float("-inf"))]
BAD_IDS = ["b", "x", "max_iter", "rtol-neg", "rtol-nan", "rtol-neg-inf"]


@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
def test_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    assert call_one(lib, plan, d=None)[0] == ERR_STATE           # a different error first: a stale text would show
    rc, msg = call_one(lib, plan, **bad)
    assert rc == ERR_ARG, bad
    assert says_one_vector(msg) and b"upload" not in msg, (bad, msg)
    assert (b"null argument" in msg) == ("b" in bad or "x" in bad), (bad, msg)
    assert (b"max_iter" in msg) == ("max_iter" in bad or "rtol" in bad), (bad, msg)


def test_null_plan(E, plan):
    lib = E.host._lib.load()
    assert call_one(lib, plan)[0] == ERR_STATE
    rc = lib.ehyb_minres(None, D, B, X, 10, 1e-8, 10, None, None, None)
    msg = lib.ehyb_last_error()
    assert rc == ERR_ARG and says_one_vector(msg) and b"null argument" in msg, msg


def test_the_order_of_the_checks(E, plan, part):
    """null argument, then max_iter / rtol, then a plan over all rows, then the upload"""
    lib = E.host._lib.load()
    rc, msg = call_one(lib, part, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"null argument" in msg
    rc, msg = call_one(lib, part, max_iter=-1)
    assert rc == ERR_ARG and b"max_iter" in msg
    rc, msg = call_one(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg and says_one_vector(msg), msg


# ------------------------------------------------------------------ ehyb_minres_multi
def test_multi_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    rc, msg = call_multi(lib, plan)
    assert rc == ERR_STATE and b"upload" in msg and b"ehyb_minres_multi" in msg
    for check_every in (0, -1):
        rc, _ = call_multi(lib, plan, ldb=plan.n + 7, ldx=plan.n + 3, k=9, max_iter=0, rtol=0.0, check_every=check_every)
        assert rc == ERR_STATE
    assert call_multi(lib, plan, d=None)[0] == ERR_STATE         # no preconditioner is fine
    assert call_multi(lib, plan, outputs=False)[0] == ERR_STATE  # so are NULL outputs
    assert call_multi(lib, plan, k=1)[0] == ERR_STATE


MULTI_BAD = [dict(b=None), dict(x=None), dict(k=0), dict(k=-2), dict(ldb=-1), dict(ldx=-1), dict(max_iter=-1), dict(rtol=-1e-9),
             dict(rtol=float("nan"))]


@pytest.mark.parametrize("bad", MULTI_BAD, ids=["B", "X", "k0", "kneg", "ldb", "ldx", "max_iter", "rtol-neg", "rtol-nan"])
def test_multi_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    bad = dict(bad)
    for ld in ("ldb", "ldx"):
        if ld in bad:
            bad[ld] = plan.n - 1
    assert call_multi(lib, plan)[0] == ERR_STATE
    rc, msg = call_multi(lib, plan, **bad)
    assert rc == ERR_ARG, bad
    assert b"ehyb_minres_multi" in msg and b"upload" not in msg, (bad, msg)


def test_multi_order_of_the_checks(E, plan, part):
    """k, then the leading dimensions, then what ehyb_minres checks in its order"""
    lib = E.host._lib.load()
    rc, msg = call_multi(lib, plan, k=0, ldb=1, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"right-hand sides" in msg, msg
    rc, msg = call_multi(lib, plan, ldb=1, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"ldb" in msg, msg
    rc, msg = call_multi(lib, plan, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"null argument" in msg, msg
    rc, msg = call_multi(lib, part, max_iter=-1)
    assert rc == ERR_ARG and b"max_iter" in msg, msg
    rc, msg = call_multi(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg and b"ehyb_minres_multi" in msg, msg
    rc = lib.ehyb_minres_multi(None, D, B, plan.n, X, plan.n, 2, 10, 1e-8, 10, None, None, None)
    assert rc == ERR_ARG and b"ehyb_minres_multi" in lib.ehyb_last_error()


# ------------------------------------------------------------------ the layout
def test_the_layout_is_consistent(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.MinresSlots()
    lib = _lib.load()
    assert lib.ehyb_minres_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert lib.ehyb_minres_layout(None) == ERR_ARG and b"ehyb_minres_layout" in lib.ehyb_last_error()
    assert out["slot_doubles"] == 1024
    named = [out["slot_bb"], out["slot_zq"], out["slot_beta0"], out["slot_beta0"] + 1]          # two beta^2 slots
    assert sorted(named) == list(range(out["slots"])), out
    state = [out["state_" + k] for k in ("dbar", "eps", "phibar", "cs", "sn", "beta_old")]
    assert sorted(state) == list(range(out["state_doubles"])), out
    # two state copies, then the flags, disjoint from them, and nothing else in the tail
    assert out["flags_at"] >= 2 * out["state_doubles"] and out["tail_doubles"] == out["flags_at"] + 1, out
    assert out["flag_count"] == 2 and sorted((out["flag_status"], out["flag_iters"])) == [0, 1], out
    assert len({out["status_running"], out["status_converged"], out["status_breakdown"]}) == 3 and out["status_running"] == 0, out


# ------------------------------------------------------------------ the step entry points
A = 0x10000
# name -> argument kinds in order: "n", "ptr" (required), "opt" (inv_diag: may be NULL), "int", "double", "stream"
STEPS = {
    "ehyb_minres_init_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "ptr", "stream"),
    "ehyb_minres_dot_step": ("n", "ptr", "ptr", "ptr", "int", "double", "stream"),
    "ehyb_minres_lanczos_step": ("n", "ptr", "ptr", "ptr", "opt", "ptr", "ptr", "int", "stream"),
    "ehyb_minres_update_step": ("n", "ptr", "opt", "ptr", "ptr", "ptr", "ptr", "int", "stream"),
}
GOOD = {"n": 100, "int": 0, "double": 1e-20, "stream": None}


def arguments(kinds, null=None, n=100, dinv=True):
    out = []
    for i, kind in enumerate(kinds):
        if kind in ("ptr", "opt"):
            out.append(None if i == null or (kind == "opt" and not dinv) else C.c_void_p(A + 0x1000 * i))
        else:
            out.append(n if kind == "n" else GOOD[kind])
    return out


def test_the_table_is_every_minres_step_function(E):
    sigs = {k: v for k, v in E.host._lib.SIGNATURES.items() if k.startswith("ehyb_minres_") and k.endswith("_step")}
    assert set(sigs) == set(STEPS)
    for name, (_, argtypes) in sigs.items():
        assert len(argtypes) == len(STEPS[name]), name


@pytest.mark.parametrize("name", sorted(STEPS))
def test_steps_reject_a_negative_n_and_a_null_pointer_they_would_use(E, name):
    lib = E.host._lib.load()
    fn, kinds = getattr(lib, name), STEPS[name]
    other = next(k for k in sorted(STEPS) if k != name)

    def stale():                          # a different error first, so that a text left over from it would be caught
        assert getattr(lib, other)(*arguments(STEPS[other], n=-1)) == ERR_ARG
        assert other.encode() in lib.ehyb_last_error()

    for i in [i for i, kind in enumerate(kinds) if kind == "ptr"]:
        for dinv in (True, False):
            stale()
            assert fn(*arguments(kinds, null=i, dinv=dinv)) == ERR_ARG, (name, i, dinv)
            msg = lib.ehyb_last_error()
            assert name.encode() + b":" in msg and other.encode() not in msg, (name, i, msg)
    for dinv in (True, False):
        stale()
        assert fn(*arguments(kinds, n=-1, dinv=dinv)) == ERR_ARG, name
        msg = lib.ehyb_last_error()
        assert name.encode() + b":" in msg and other.encode() not in msg, (name, msg)
