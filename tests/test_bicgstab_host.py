"""ehyb_bicgstab and ehyb_pcg on the host: every argument check of the two one-vector solves (the same C signature), on plans
that were never uploaded -- the checks come before any device work, so nothing here needs a GPU."""
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


B, X, D = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)   # never read: every call fails before device work
SOLVERS = ["ehyb_bicgstab", "ehyb_pcg"]


def call(lib, plan, who, h=None, d=D, b=B, x=X, max_iter=50, rtol=1e-8, check_every=10, outputs=True):
    it, rel = C.c_int(-5), C.c_double(-5.0)
    h = plan.h if h is None else h
    rc = getattr(lib, who)(h, d, b, x, max_iter, rtol, check_every, None, C.byref(it) if outputs else None,
                           C.byref(rel) if outputs else None)
    return rc, lib.ehyb_last_error()


@pytest.mark.parametrize("who", SOLVERS)
def test_never_uploaded_plan_is_a_state_error(E, plan, who):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan, who)
    assert rc == ERR_STATE and b"upload" in msg and who.encode() in msg
    # zero iterations, rtol = 0, check_every <= 0, no preconditioner, no outputs: still only the upload is missing
    for kw in (dict(max_iter=0), dict(rtol=0.0), dict(check_every=0), dict(check_every=-3), dict(d=None), dict(outputs=False)):
        rc, _ = call(lib, plan, who, **kw)
        assert rc == ERR_STATE, kw


BAD = [dict(b=None), dict(x=None), dict(max_iter=-1), dict(rtol=-1e-9), dict(rtol=float("nan")), dict(rtol=float("-inf"))]
BAD_IDS = ["b", "x", "max_iter", "rtol-neg", "rtol-nan", "rtol-neg-inf"]
# ids: the bad argument alone for ehyb_bicgstab, prefixed with the entry point for the others
CASES = [pytest.param(who, bad, id=i if who == "ehyb_bicgstab" else f"{who}-{i}") for who in SOLVERS for bad, i in zip(BAD, BAD_IDS)]


@pytest.mark.parametrize("who,bad", CASES)
def test_argument_errors_come_before_the_state_error(E, plan, who, bad):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan, who, **bad)
    assert rc == ERR_ARG, bad
    assert who.encode() in msg, (bad, msg)


@pytest.mark.parametrize("who", SOLVERS)
def test_null_plan(E, who):
    lib = E.host._lib.load()
    rc = getattr(lib, who)(None, D, B, X, 10, 1e-8, 10, None, None, None)
    assert rc == ERR_ARG and lib.ehyb_last_error()


@pytest.mark.parametrize("who", SOLVERS)
def test_plan_over_some_rows_is_refused(E, who):
    lib = E.host._lib.load()
    part = host_plan(E, half=True, direct=2)
    assert 0 < part.rows[1] < part.n
    rc, msg = call(lib, part, who)
    assert rc == ERR_ARG and b"all rows" in msg
    rc, _ = call(lib, part, who, max_iter=-1)
    assert rc == ERR_ARG

