"""ehyb_bicgstab_multi and ehyb_bicgstab on the host: every argument check of the k-right-hand-side BiCGSTAB and of the one-vector
entry point onto the same driver, on plans that were never uploaded -- the checks come before any device work, so nothing here
needs a GPU."""
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
    return host_plan(E, direct=2, sym_pairs=0)


B, X, D = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)   # never read: every call fails before device work


def call(lib, plan, h=None, d=D, b=B, ldb=None, x=X, ldx=None, k=3, max_iter=50, rtol=1e-8, check_every=10, outputs=True):
    n = plan.n
    it = (C.c_int * 16)() if outputs else None
    rel = (C.c_double * 16)() if outputs else None
    h = plan.h if h is None else h
    ldb = n if ldb is None else ldb
    ldx = n if ldx is None else ldx
    rc = lib.ehyb_bicgstab_multi(h, d, b, ldb, x, ldx, k, max_iter, rtol, check_every, None, it, rel)
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan)
    assert rc == ERR_STATE and b"upload" in msg and b"ehyb_bicgstab_multi" in msg
    # wide leading dimensions, many columns, zero iterations, check_every <= 0: still only the upload is missing
    for check_every in (0, -1):
        rc, _ = call(lib, plan, ldb=plan.n + 7, ldx=plan.n + 3, k=9, max_iter=0, rtol=0.0, check_every=check_every)
        assert rc == ERR_STATE
    rc, _ = call(lib, plan, d=None)                  # no preconditioner is fine
    assert rc == ERR_STATE
    rc, _ = call(lib, plan, outputs=False)           # so are NULL outputs
    assert rc == ERR_STATE


BAD = [dict(b=None), dict(x=None), dict(k=0), dict(k=-2), dict(ldb=-1), dict(ldx=-1),
       dict(max_iter=-1), dict(rtol=-1e-9), dict(rtol=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=["B", "X", "k0", "kneg", "ldb", "ldx", "max_iter", "rtol-neg", "rtol-nan"])
def test_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    bad = dict(bad)
    if "ldb" in bad:
        bad["ldb"] = plan.n - 1
    if "ldx" in bad:
        bad["ldx"] = plan.n - 1
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG, bad
    assert b"ehyb_bicgstab_multi" in msg, (bad, msg)


def test_null_plan(E, plan):
    lib = E.host._lib.load()
    rc = lib.ehyb_bicgstab_multi(None, D, B, plan.n, X, plan.n, 2, 10, 1e-8, 10, None, None, None)
    assert rc == ERR_ARG and b"ehyb_bicgstab_multi" in lib.ehyb_last_error()


def test_plan_over_some_rows_is_refused(E):
    lib = E.host._lib.load()
    part = host_plan(E, half=True, direct=2, sym_pairs=0)
    assert 0 < part.rows[1] < part.n
    rc, msg = call(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg


# ------------------------------------------------------------------ the one-vector entry point: the same driver, its own name
def call_one(lib, plan, h=None, d=D, b=B, x=X, max_iter=50, rtol=1e-8, check_every=10, outputs=True):
    it, rel = (C.c_int(0), C.c_double(0)) if outputs else (None, None)
    rc = lib.ehyb_bicgstab(plan.h if h is None else h, d, b, x, max_iter, rtol, check_every, None,
                           C.byref(it) if outputs else None, C.byref(rel) if outputs else None)
    return rc, lib.ehyb_last_error()


def says_one_vector(msg):
    return b"ehyb_bicgstab:" in msg and b"_multi" not in msg


def test_one_vector_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    rc, msg = call_one(lib, plan)
    assert rc == ERR_STATE and b"upload" in msg and says_one_vector(msg), msg
    for kw in (dict(max_iter=0, rtol=0.0, check_every=0), dict(max_iter=0, rtol=0.0, check_every=-1), dict(d=None),
               dict(outputs=False), dict(d=None, outputs=False, max_iter=0, check_every=0)):
        rc, msg = call_one(lib, plan, **kw)
        assert rc == ERR_STATE and says_one_vector(msg), (kw, msg)


@pytest.mark.parametrize("bad", [dict(b=None), dict(x=None), dict(max_iter=-1), dict(rtol=-1e-9), dict(rtol=float("nan"))],
                         ids=["b", "x", "max_iter", "rtol-neg", "rtol-nan"])
def test_one_vector_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    assert call_one(lib, plan, d=None)[0] == ERR_STATE           # a different error first: a stale text would show
    rc, msg = call_one(lib, plan, **bad)
    assert rc == ERR_ARG, bad
    assert says_one_vector(msg) and b"upload" not in msg, (bad, msg)
    assert (b"null argument" in msg) == ("b" in bad or "x" in bad), (bad, msg)
    assert (b"max_iter" in msg) == ("max_iter" in bad or "rtol" in bad), (bad, msg)


def test_one_vector_null_plan(E, plan):
    lib = E.host._lib.load()
    assert call_one(lib, plan)[0] == ERR_STATE
    rc = lib.ehyb_bicgstab(None, D, B, X, 10, 1e-8, 10, None, None, None)
    msg = lib.ehyb_last_error()
    assert rc == ERR_ARG and says_one_vector(msg) and b"null argument" in msg, msg


def test_one_vector_plan_over_some_rows_is_refused(E):
    lib = E.host._lib.load()
    part = host_plan(E, half=True, direct=2, sym_pairs=0)
    rc, msg = call_one(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg and says_one_vector(msg), msg
