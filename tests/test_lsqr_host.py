"""ehyb_lsqr on the host: the numpy restatement lsqr_cases.cpu_lsqr against scipy.sparse.linalg.lsqr on the six test systems,
the exact step cases' own consistency, Matrix.transposed_like and pad_square, the published layout, and every argument check of
ehyb_lsqr / ehyb_lsqr_multi / the step entry points in the order of the header, on plans that were never uploaded -- all before
any device work, so nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import lsqr_cases as lc
import solver_cases as sc

ERR_ARG, ERR_STATE = 1, 8                # EHYB_ERR_ARG, EHYB_ERR_STATE
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
FEM_OTHER = ("fem3d", (12000, 3, 22, 22, 13500, 1, 1))


# ------------------------------------------------------------------ the yardstick itself
@pytest.fixture(scope="module")
def systems():
    return lc.systems()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_the_restatement_against_scipy(systems, name):
    """same istop, iteration counts within 2, x within 1e-8 relative, the four estimates within 1e-6; the padded entries of x are
    exactly +0.0"""
    s = systems[name]
    m, n = s["shape"]
    x, info = lc.cpu_lsqr(s["Asq"], s["b"], damp=s["damp"], atol=1e-10, btol=1e-10, max_iter=1000)
    ref = spla.lsqr(s["A"], s["b"][:m], damp=s["damp"], atol=1e-10, btol=1e-10, conlim=0, iter_lim=1000)
    err = np.linalg.norm(x[:n] - ref[0]) / max(np.linalg.norm(ref[0]), 1e-300)
    print(name, info, "scipy", ref[1], ref[2], "error", err)
    assert info["istop"] == ref[1] and abs(info["iters"] - ref[2]) <= 2, (info, ref[1:3])
    assert err <= 1e-8, err
    assert np.array_equal(x[n:].view(np.int64), np.zeros(lc.N - n).view(np.int64))
    if name not in ("e", "f"):          # (e) ends at rounding level, where the estimates are noise
        for key, at in (("rnorm", 4), ("anorm", 5), ("arnorm", 7), ("xnorm", 8)):
            assert abs(info[key] - ref[at]) <= 1e-6 * abs(ref[at]), (key, info[key], ref[at])
    assert {"a": 1, "b": 2, "c": 2, "d": 1, "e": 1, "f": 0}[name] == info["istop"]
    if name == "e":
        assert info["iters"] == 2
    if name == "f":
        assert info["iters"] == 0 and not x.any()


def test_the_restatement_solves_what_it_says(systems):
    """(b) against numpy.linalg.lstsq, (c) against the normal equations, (d) against the minimum-norm solution"""
    s = systems["b"]
    T = s["A"].toarray()
    x, _ = lc.cpu_lsqr(s["Asq"], s["b"])
    want = np.linalg.lstsq(T, s["b"], rcond=None)[0]
    assert np.linalg.norm(x[:lc.M_COLS] - want) <= 1e-8 * np.linalg.norm(want)
    x, _ = lc.cpu_lsqr(s["Asq"], s["b"], damp=0.5)
    want = np.linalg.solve(T.T @ T + 0.25 * np.eye(lc.M_COLS), T.T @ s["b"])
    assert np.linalg.norm(x[:lc.M_COLS] - want) <= 1e-8 * np.linalg.norm(want)
    s = systems["d"]
    x, _ = lc.cpu_lsqr(s["Asq"], s["b"])
    want = np.linalg.pinv(s["A"].toarray()) @ s["b"][:lc.M_COLS]
    assert np.linalg.norm(x - want) <= 1e-8 * np.linalg.norm(want)


def test_the_restatement_breaks_down_on_a_nan(systems):
    s = systems["a"]
    b = s["b"].copy()
    b[7] = np.nan
    x0 = np.arange(lc.N, dtype=np.float64)
    x, info = lc.cpu_lsqr(s["Asq"], b, x0=x0)
    assert info["istop"] == -1 and info["iters"] == 0 and np.array_equal(x, x0)


def test_the_exact_cases_build_at_every_size():
    """every case asserts its own exactness while it is built (Fx.f, partials, _ex)"""
    for n in (0, 1, 257, sc.S + 1):
        lc.lsqr_init_case(n)
        for cur in (0, 1):
            lc.lsqr_start_case(n, cur)
            lc.lsqr_wstart_case(n, cur)
            lc.lsqr_pair_case(n, cur)
            for lucky in (None, "beta", "alpha"):
                c = lc.lsqr_update_case(n, cur, lucky)
                assert ("w" in c["out"]) == (lucky is None)
                assert all(np.isfinite(v) for v in c["scalars"]["state_new"].values())


# ------------------------------------------------------------------ transposed_like, pad_square
def test_transposed_like_is_the_transpose_in_the_same_numbering(E):
    A = lc.convection(12, 9)
    cfg = E.make_config(window_mode=2, lds_doubles=32, sym_pairs=0)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=False)
    m.reorder(cfg)
    assert m.c.nParts > 1 and not np.array_equal(m.reorder_list, np.arange(m.n)), "the case must permute"
    t = m.transposed_like(cfg)
    assert (t.to_scipy() != m.to_scipy().T).nnz == 0
    assert np.array_equal(t.part_boundary, m.part_boundary) and np.array_equal(t.reorder_list, m.reorder_list)
    plan = E.Plan(t, E.make_config(window_mode=2, lds_doubles=32, sym_pairs=2), upload=False)
    assert plan.n == m.n


def test_pad_square(E):
    T = sp.random(7, 4, density=0.5, random_state=np.random.default_rng(1)).tocsr()
    for A in (T, T.T.tocsr()):
        indptr, indices, data = E.pad_square(A.indptr, A.indices, A.data, A.shape)
        got = sp.csr_matrix((data, indices, indptr), shape=(7, 7))
        assert (got != lc.padded(A)).nnz == 0
        m = E.Matrix.from_csr(indptr, indices, data, None, symmetric=False)
        assert m.n == 7 and m.nnz == A.nnz


# ------------------------------------------------------------------ the argument checks
def host_plan(E, gen=FEM_SMALL, half=False, **kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    m.reorder(cfg)
    pb = m.part_boundary
    return E.Plan(m, cfg, rows=(0, int(pb[len(pb) // 2])) if half else None, upload=False)


@pytest.fixture(scope="module")
def plan(E):
    p = host_plan(E, direct=2, sym_pairs=0)
    assert p.spmv_t_supported
    return p


@pytest.fixture(scope="module")
def part(E):
    p = host_plan(E, half=True, direct=2, sym_pairs=0)
    assert 0 < p.rows[1] < p.n
    return p


@pytest.fixture(scope="module")
def other(E):
    return host_plan(E, gen=FEM_OTHER, direct=2, sym_pairs=0)


@pytest.fixture(scope="module")
def pairs(E):
    p = host_plan(E, direct=2, sym_pairs=1)
    assert not p.spmv_t_supported
    return p


B, X = C.c_void_p(0x10000), C.c_void_p(0x20000)   # never read: every call fails before device work


def call_one(lib, plan, plan_t=None, b=B, x=X, damp=0.0, atol=1e-8, btol=1e-8, max_iter=50, check_every=10, info=True):
    from ehyb_spmv_gpu_amd import _lib

    out = _lib.LsqrInfo()
    rc = lib.ehyb_lsqr(plan.h if plan is not None else None, plan_t.h if plan_t is not None else None, b, x, damp, atol, btol, max_iter,
                       check_every, None, C.byref(out) if info else None)
    return rc, lib.ehyb_last_error()


def call_multi(lib, plan, plan_t=None, b=B, ldb=None, x=X, ldx=None, k=3, damp=0.0, atol=1e-8, btol=1e-8, max_iter=50, check_every=10):
    n = plan.n
    rc = lib.ehyb_lsqr_multi(plan.h, plan_t.h if plan_t is not None else None, b, n if ldb is None else ldb, x, n if ldx is None else ldx, k,
                             damp, atol, btol, max_iter, check_every, None, None)
    return rc, lib.ehyb_last_error()


def says_one_vector(msg):
    return b"ehyb_lsqr:" in msg and b"_multi" not in msg


def test_never_uploaded_plans_are_state_errors(E, plan, part):
    lib = E.host._lib.load()
    rc, msg = call_one(lib, plan)
    assert rc == ERR_STATE and b"plan not uploaded" in msg and says_one_vector(msg), msg
    rc, msg = call_one(lib, plan, plan_t=plan)
    assert rc == ERR_STATE and b"plan not uploaded" in msg, msg
    for kw in (dict(max_iter=0), dict(atol=0.0, btol=0.0), dict(damp=2.5), dict(check_every=0), dict(check_every=-3), dict(info=False)):
        rc, msg = call_one(lib, plan, **kw)
        assert rc == ERR_STATE and says_one_vector(msg), (kw, msg)


BAD = [dict(b=None), dict(x=None), dict(max_iter=-1), dict(damp=-1.0), dict(damp=float("nan")), dict(atol=-1e-9), dict(atol=float("nan")),
       dict(btol=-1e-9), dict(btol=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=["b", "x", "max_iter", "damp-neg", "damp-nan", "atol-neg", "atol-nan", "btol-neg", "btol-nan"])
def test_argument_errors_come_before_the_state_error(E, plan, bad):
    lib = E.host._lib.load()
    assert call_one(lib, plan)[0] == ERR_STATE                   # a different error first: a stale text would show
    rc, msg = call_one(lib, plan, **bad)
    assert rc == ERR_ARG and says_one_vector(msg) and b"upload" not in msg, (bad, msg)
    assert (b"null argument" in msg) == ("b" in bad or "x" in bad), (bad, msg)
    assert (b"max_iter" in msg) == ("max_iter" in bad), (bad, msg)
    assert (b"damp" in msg and b"atol" in msg) == bool({"damp", "atol", "btol"} & set(bad)), (bad, msg)


def test_the_order_of_the_checks(E, plan, part, other, pairs):
    """null argument, max_iter, the tolerances, a plan over all rows, the plan_t's dimension and rows, the spmv_t refusal, then
    the uploads"""
    lib = E.host._lib.load()
    rc, msg = call_one(lib, None, max_iter=-1)
    assert rc == ERR_ARG and b"null argument" in msg and says_one_vector(msg), msg
    rc, msg = call_one(lib, part, plan_t=other, b=None, max_iter=-1, damp=-1.0)
    assert rc == ERR_ARG and b"null argument" in msg
    rc, msg = call_one(lib, part, plan_t=other, max_iter=-1, damp=-1.0)
    assert rc == ERR_ARG and b"max_iter" in msg
    rc, msg = call_one(lib, part, plan_t=other, damp=-1.0)
    assert rc == ERR_ARG and b"damp" in msg
    rc, msg = call_one(lib, part, plan_t=other)
    assert rc == ERR_ARG and b"all rows" in msg and b"plan_t" not in msg, msg
    rc, msg = call_one(lib, plan, plan_t=other)
    assert rc == ERR_ARG and b"plan_t has" in msg and says_one_vector(msg), msg
    rc, msg = call_one(lib, plan, plan_t=part)
    assert rc == ERR_ARG and b"plan_t over all rows" in msg, msg
    # plan_t NULL on symmetric pair storage: ehyb_spmv_t_supported's own message; with plan_t == plan it goes through
    rc, msg = call_one(lib, pairs)
    assert rc == ERR_ARG and b"ehyb_spmv_t: not built for" in msg, msg
    assert pairs.spmv_t_refusal[1].encode() == msg
    rc, msg = call_one(lib, pairs, plan_t=pairs)
    assert rc == ERR_STATE and b"plan not uploaded" in msg, msg


def test_multi_order_of_the_checks(E, plan, part, other):
    """k, then the leading dimensions, then what ehyb_lsqr checks in its order"""
    lib = E.host._lib.load()
    rc, msg = call_multi(lib, plan, k=0, ldb=1, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"right-hand sides" in msg and b"ehyb_lsqr_multi" in msg, msg
    for ld in ("ldb", "ldx"):
        rc, msg = call_multi(lib, plan, b=None, max_iter=-1, **{ld: plan.n - 1})
        assert rc == ERR_ARG and b"ldb" in msg, msg
    rc, msg = call_multi(lib, plan, b=None, max_iter=-1)
    assert rc == ERR_ARG and b"null argument" in msg, msg
    rc, msg = call_multi(lib, part, max_iter=-1, atol=-1.0)
    assert rc == ERR_ARG and b"max_iter" in msg, msg
    rc, msg = call_multi(lib, part, atol=-1.0)
    assert rc == ERR_ARG and b"atol" in msg, msg
    rc, msg = call_multi(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg and b"ehyb_lsqr_multi" in msg, msg
    rc, msg = call_multi(lib, plan, plan_t=other)
    assert rc == ERR_ARG and b"plan_t has" in msg, msg
    rc, msg = call_multi(lib, plan, ldb=plan.n + 7, ldx=plan.n + 3, k=9, max_iter=0)
    assert rc == ERR_STATE and b"ehyb_lsqr_multi" in msg, msg
    rc = lib.ehyb_lsqr_multi(None, None, B, plan.n, X, plan.n, 2, 0.0, 1e-8, 1e-8, 10, 10, None, None)
    assert rc == ERR_ARG and b"ehyb_lsqr_multi" in lib.ehyb_last_error()


# ------------------------------------------------------------------ the layout
def test_the_layout_is_consistent_and_needs_no_device(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.LsqrSlots()
    lib = _lib.load()
    assert lib.ehyb_lsqr_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert lib.ehyb_lsqr_layout(None) == ERR_ARG and b"ehyb_lsqr_layout" in lib.ehyb_last_error()
    assert out["slot_doubles"] == 1024
    named = [out["slot_bb"], out["slot_beta0"], out["slot_beta0"] + 1, out["slot_alpha0"], out["slot_alpha0"] + 1]
    assert sorted(named) == list(range(out["slots"])), out
    assert sorted(out["state_" + k] for k in lc.STATE) == list(range(out["state_doubles"])), out
    assert out["flags_at"] >= 2 * out["state_doubles"] and out["tail_doubles"] == out["flags_at"] + 1, out
    assert out["flag_count"] == 2 and sorted((out["flag_status"], out["flag_iters"])) == [0, 1], out
    assert len({out["status_running"], out["status_converged"], out["status_breakdown"]}) == 3 and out["status_running"] == 0, out
    assert C.sizeof(_lib.LsqrInfo) == 40


# ------------------------------------------------------------------ the step entry points
A = 0x10000
STEPS = {
    "ehyb_lsqr_init_step": ("n", "k", "ptr", "ptr", "ptr", "ptr", "stream"),
    "ehyb_lsqr_start_step": ("n", "k", "ptr", "ptr", "ptr", "stream"),
    "ehyb_lsqr_wstart_step": ("n", "k", "ptr", "ptr", "ptr", "stream"),
    "ehyb_lsqr_ustep_step": ("n", "k", "ptr", "ptr", "ptr", "int", "double", "double", "stream"),
    "ehyb_lsqr_vstep_step": ("n", "k", "ptr", "ptr", "ptr", "int", "stream"),
    "ehyb_lsqr_update_step": ("n", "k", "ptr", "ptr", "ptr", "ptr", "int", "double", "stream"),
}
GOOD = {"int": 0, "double": 1e-20, "stream": None}


def arguments(kinds, null=None, n=100, k=1):
    out = []
    for i, kind in enumerate(kinds):
        if kind == "ptr":
            out.append(None if i == null else C.c_void_p(A + 0x1000 * i))
        else:
            out.append(n if kind == "n" else k if kind == "k" else GOOD[kind])
    return out


def test_the_table_is_every_lsqr_step_function(E):
    sigs = {k: v for k, v in E.host._lib.SIGNATURES.items() if k.startswith("ehyb_lsqr_") and k.endswith("_step")}
    assert set(sigs) == set(STEPS)
    for name, (_, argtypes) in sigs.items():
        assert len(argtypes) == len(STEPS[name]), name


@pytest.mark.parametrize("name", sorted(STEPS))
def test_steps_reject_a_negative_n_a_null_pointer_and_a_bad_k(E, name):
    lib = E.host._lib.load()
    fn, kinds = getattr(lib, name), STEPS[name]
    other = next(k for k in sorted(STEPS) if k != name)

    def stale():                          # a different error first, so that a text left over from it would be caught
        assert getattr(lib, other)(*arguments(STEPS[other], n=-1)) == ERR_ARG
        assert other.encode() in lib.ehyb_last_error()

    bad = [dict(null=i) for i, kind in enumerate(kinds) if kind == "ptr"] + [dict(n=-1), dict(k=0), dict(k=5), dict(k=-1)]
    for kw in bad:
        stale()
        assert fn(*arguments(kinds, **kw)) == ERR_ARG, (name, kw)
        msg = lib.ehyb_last_error()
        assert name.encode() + b":" in msg and other.encode() not in msg, (name, kw, msg)
