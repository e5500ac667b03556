"""ehyb_gmres, ehyb_gmres_layout and the ehyb_gmres_*_step building blocks on the host: every argument check and their order on
plans that were never uploaded, the consistency of the published layout, and the step entry points' own checks -- all before any
device work, so nothing here needs a GPU."""
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


def call(lib, plan, d=D, b=B, x=X, restart=30, passes=2, max_iter=50, rtol=1e-8, outputs=True):
    it, rel = C.c_int(-5), C.c_double(-5.0)
    rc = lib.ehyb_gmres(plan.h, d, b, x, restart, passes, max_iter, rtol, None, C.byref(it) if outputs else None,
                        C.byref(rel) if outputs else None)
    assert (it.value, rel.value) == (-5, -5.0), "an output was written before device work"
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan)
    assert rc == ERR_STATE and b"upload" in msg and b"ehyb_gmres:" in msg, msg
    # every restart and pass count the header allows, zero iterations, rtol = 0, no preconditioner, no outputs
    for kw in (dict(restart=0), dict(restart=1), dict(restart=64), dict(passes=0), dict(passes=1), dict(max_iter=0), dict(rtol=0.0),
               dict(d=None), dict(outputs=False), dict(d=None, outputs=False, max_iter=0, restart=0, passes=0)):
        rc, msg = call(lib, plan, **kw)
        assert rc == ERR_STATE and b"ehyb_gmres:" in msg, (kw, msg)


BAD = [dict(b=None), dict(x=None), dict(max_iter=-1), dict(rtol=-1e-9), dict(rtol=float("nan")), dict(rtol=float("-inf")),
       dict(restart=65), dict(restart=-1), dict(passes=3), dict(passes=-1)]
BAD_IDS = ["b", "x", "max_iter", "rtol-neg", "rtol-nan", "rtol-neg-inf", "restart-65", "restart-neg", "passes-3", "passes-neg"]


@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
def test_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    assert call(lib, plan, d=None)[0] == ERR_STATE               # a different error first: a stale text would show
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG, bad
    assert b"ehyb_gmres:" in msg and b"upload" not in msg, (bad, msg)
    assert (b"null argument" in msg) == ("b" in bad or "x" in bad), (bad, msg)
    assert (b"max_iter" in msg) == ("max_iter" in bad or "rtol" in bad), (bad, msg)
    assert (b"restart" in msg) == ("restart" in bad or "passes" in bad), (bad, msg)


def test_null_plan(E, plan):
    lib = E.host._lib.load()
    assert call(lib, plan)[0] == ERR_STATE
    rc = lib.ehyb_gmres(None, D, B, X, 30, 2, 10, 1e-8, None, None, None)
    msg = lib.ehyb_last_error()
    assert rc == ERR_ARG and b"ehyb_gmres:" in msg and b"null argument" in msg, msg


def test_the_order_of_the_checks(E, plan, part):
    """null argument, then max_iter / rtol, then a plan over all rows, then restart / ortho_passes, then the upload"""
    lib = E.host._lib.load()
    rc, msg = call(lib, part, b=None, max_iter=-1, restart=65)
    assert rc == ERR_ARG and b"null argument" in msg
    rc, msg = call(lib, part, max_iter=-1, restart=65)
    assert rc == ERR_ARG and b"max_iter" in msg
    rc, msg = call(lib, part, restart=65, passes=3)
    assert rc == ERR_ARG and b"all rows" in msg and b"ehyb_gmres:" in msg, msg
    rc, msg = call(lib, plan, restart=65)
    assert rc == ERR_ARG and b"restart" in msg, msg
    rc, msg = call(lib, plan, passes=3)
    assert rc == ERR_ARG and b"ortho_passes" in msg, msg
    assert call(lib, plan)[0] == ERR_STATE


# ------------------------------------------------------------------ the layout
def test_the_layout_is_consistent(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.GmresSlots()
    lib = _lib.load()
    assert lib.ehyb_gmres_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert lib.ehyb_gmres_layout(None) == ERR_ARG and b"ehyb_gmres_layout" in lib.ehyb_last_error()
    m = out["max_restart"]
    assert out["slot_doubles"] == 1024 and m == 64
    # b.b, w.w and one slot per basis column (max_restart + 1 of them), nothing else
    assert sorted([out["slot_bb"], out["slot_ww"]] + list(range(out["slot_c0"], out["slot_c0"] + m + 1))) == list(range(out["slots"])), out
    # the tail: its pieces are disjoint and fill it
    pieces = [(out["flags_at"], 1), (out["cycle_at"], 1), (out["rho_at"], 1), (out["bb_at"], 1), (out["cs_at"], m), (out["sn_at"], m),
              (out["gt_at"], m + 1), (out["g_at"], m), (out["h_at"], 2 * out["h_stride"]), (out["r_at"], m * out["r_stride"])]
    covered = sorted(i for at, count in pieces for i in range(at, at + count))
    assert covered == list(range(out["tail_doubles"])), out
    assert out["h_stride"] >= m + 1 and out["r_stride"] >= m
    assert out["flag_count"] == 2 and sorted((out["flag_status"], out["flag_iters"])) == [0, 1], out
    assert len({out["status_running"], out["status_converged"], out["status_breakdown"]}) == 3 and out["status_running"] == 0, out


# ------------------------------------------------------------------ the step entry points
A = 0x10000
# name -> argument kinds in order: "n", "ld", "ptr" (required), "opt" (inv_diag: may be NULL), "count", "int", "j", "passes",
# "double", "stream"
STEPS = {
    "ehyb_gmres_start_step": ("n", "ptr", "ptr", "ptr", "stream"),
    "ehyb_gmres_dots_step": ("n", "ld", "ptr", "ptr", "count", "ptr", "stream"),
    "ehyb_gmres_update_step": ("n", "ld", "ptr", "ptr", "count", "ptr", "int", "int", "stream"),
    "ehyb_gmres_next_step": ("n", "ld", "ptr", "ptr", "opt", "ptr", "ptr", "j", "passes", "double", "stream"),
    "ehyb_gmres_solve_x_step": ("n", "ld", "ptr", "opt", "ptr", "ptr", "stream"),
}
GOOD = {"n": 100, "ld": 100, "count": 3, "int": 0, "j": 2, "passes": 2, "double": 1e-20, "stream": None}


def arguments(kinds, null=None, dinv=True, **over):
    out = []
    for i, kind in enumerate(kinds):
        if kind in ("ptr", "opt"):
            out.append(None if i == null or (kind == "opt" and not dinv) else C.c_void_p(over.get("ptr", A + 0x1000 * i)))
        else:
            out.append(over.get(kind, GOOD[kind]))
    return out


def test_the_table_is_every_gmres_step_function(E):
    sigs = {k: v for k, v in E.host._lib.SIGNATURES.items() if k.startswith("ehyb_gmres_") and k.endswith("_step")}
    assert set(sigs) == set(STEPS)
    for name, (_, argtypes) in sigs.items():
        assert len(argtypes) == len(STEPS[name]), name


@pytest.mark.parametrize("name", sorted(STEPS))
def test_steps_reject_what_they_cannot_use(E, name):
    """a negative n, a null pointer they would use, and -- where they take them -- an odd or short leading dimension, a misaligned
    vector and a count, pass, j or passes outside its range; never inv_diag = NULL"""
    lib = E.host._lib.load()
    fn, kinds = getattr(lib, name), STEPS[name]
    other = next(k for k in sorted(STEPS) if k != name)

    def stale():                          # a different error first, so that a text left over from it would be caught
        assert getattr(lib, other)(*arguments(STEPS[other], n=-1)) == ERR_ARG
        assert other.encode() in lib.ehyb_last_error()

    def rejected(what, *args):
        stale()
        assert fn(*args) == ERR_ARG, (name, what)
        msg = lib.ehyb_last_error()
        assert name.encode() + b":" in msg and other.encode() not in msg, (name, what, msg)

    for i in [i for i, kind in enumerate(kinds) if kind == "ptr"]:
        for dinv in (True, False):
            rejected(("null", i, dinv), *arguments(kinds, null=i, dinv=dinv))
    for dinv in (True, False):
        rejected("n", *arguments(kinds, n=-1, dinv=dinv))
    if "ld" in kinds:
        rejected("odd ld", *arguments(kinds, ld=101))
        rejected("short ld", *arguments(kinds, ld=98))
        rejected("misaligned", *arguments(kinds, ptr=A + 8))
    bad = {"count": (0, 66), "j": (-2, 64), "passes": (0, 3)}
    for kind, values in bad.items():
        if kind in kinds:
            for v in values:
                rejected((kind, v), *arguments(kinds, **{kind: v}))
    if name == "ehyb_gmres_update_step":
        args = arguments(kinds)
        args[6] = 2                       # pass
        rejected("pass 2", *args)
