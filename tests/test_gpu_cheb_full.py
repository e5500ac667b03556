"""The Chebyshev solver (ehyb_cheb.hip) at the size where every loop of its kernels runs: BigSystem of
test_gpu_solver_kernels.py, n = 943,104 -- the solve launches 512 workgroups like the *_step entry points, every thread of
cheb_multi_start_kernel<K> and cheb_multi_step_kernel<K> runs the four-stride unrolled body (walk profiles (1,3) and (2,0))
and every thread of the two lambda kernels makes seven or eight trips.  At the 12,000 rows of test_gpu_cheb.py no thread
enters an unrolled body or makes a second trip.

  - ehyb_pcg_cheb_multi against ehyb_pcg_cheb column by column for column groups of 2, 3 and 4, on a bank whose columns freeze
    before the first iteration, at check points 2, 4 and 6 and never (cheb_cases.MIX_E; asserted from iters_done), while the
    polynomial's multiplies keep going over the frozen ones; degrees 4 (Jacobi scaling), 2 (none), 1 and 0; the polynomial on
    the cfg.val_f32 plan; ldb > n, ldx > n and X0 != 0 through the C entry point; a caller's stream;
  - ehyb_pcg_cheb as the composition of its own kernels (ehyb_cheb_start_step, ehyb_cheb_step and the CG steps, each tested
    exactly one launch at a time in test_gpu_cheb_kernels.py and test_gpu_solver_kernels.py) with the coefficients of
    ehyb_cheb_coeffs: a wrong slot number, parity or w_in that still converges shows here;
  - ehyb_lambda_max against the restatement.

Everything is compared bit for bit (view(np.int64)); the two tolerances that appear are those of the tests of
test_gpu_cheb.py they restate at this size (test_degree_zero_is_scaled_jacobi, test_lambda_max_is_a_lower_estimate)."""
import ctypes as C
import math

import numpy as np
import pytest

import cheb_cases as cc
import solver_cases as sc
from solver_cases import MAX_GRID, SENTINEL
from test_gpu_solver_kernels import (BIG_SPD_KW, COMPOSED_M, MIX_EVERY, MIX_ITERS, MIX_KINDS, MIX_RTOL, NEVER,  # noqa: F401
                                     assert_columns_same_bits, assert_solve_same_bits, assert_the_mix, big_spd, cg_layout, device)

pytestmark = pytest.mark.gpu

DEGREE = 4
LMAX_JACOBI = 2.1            # the power method gives 1.910 after 20 steps, Gershgorin 1.993


class ChebSystem:
    """big_spd, the cfg.val_f32 plan of its reordered matrix, the bank of cheb_cases.mix_bank with the start vectors of every
    (degree, Jacobi) of cheb_cases.MIX_E, and the one-vector solves computed so far"""

    def __init__(self, E, s):
        self.E, self.s, self.n = E, s, s.n
        self.plan, self.plain_launches, self.inv_diag = s.plan, s.plain_launches, s.inv_diag
        self.f32 = E.Plan(s.m, E.make_config(val_f32=1, **BIG_SPD_KW))
        assert self.plan.spmm_max_k == 4 and self.f32.spmm_max_k == 1 and self.f32.stats == self.plan.stats
        assert self.f32.device_value_bytes[0] == 4 * len(self.f32.array("ell_val")) > 0
        self.rowsum = np.asarray(abs(s.A).sum(axis=1)).ravel()
        self.lmax_plain = 1.05 * float(self.rowsum.max())
        self.x_star, B, self.U, self.rank = cc.mix_bank(s.A, MIX_KINDS)
        self.B = np.stack([E.vector_reorder(b, s.perm) for b in B])
        assert np.array_equal(self.B.view(np.int64), s.B.view(np.int64)), "the right-hand sides are those of big_spd"
        self.banks, self.singles = {}, {}

    def X0(self, degree, jacobi):
        if (degree, jacobi) not in self.banks:
            x0 = cc.mix_x0(self.x_star, self.U, self.rank, cc.MIX_E[degree, jacobi])
            self.banks[degree, jacobi] = np.stack([self.E.vector_reorder(x, self.s.perm) for x in x0])
        return self.banks[degree, jacobi]

    def kw(self, jacobi, f32=False, lmin=0.0, lmax=None):
        return dict(poly_plan=self.f32 if f32 else None, lmin=lmin, lmax=lmax or (LMAX_JACOBI if jacobi else self.lmax_plain),
                    max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY, inv_diag=self.inv_diag if jacobi else None)

    def single_solves(self, k, degree, jacobi, f32=False, lmin=0.0, lmax=None):
        X0, out = self.X0(degree, jacobi), []
        for j in range(k):
            key = (degree, jacobi, f32, lmin, lmax, j)
            if key not in self.singles:
                self.singles[key] = self.plan.cg_cheb(self.B[j], degree, x0=X0[j], **self.kw(jacobi, f32, lmin, lmax))
            out.append(self.singles[key])
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


@pytest.fixture(scope="module")
def cheb_sys(E, gpu, big_spd):  # noqa: F811
    return ChebSystem(E, big_spd)


# ------------------------------------------------------------------ k columns against one
@pytest.mark.parametrize("degree,jacobi", [(DEGREE, True), (2, False)], ids=["degree4-jacobi", "degree2-plain"])
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_wide_cheb_kernels_at_full_size_equal_the_single_solve(E, gpu, cheb_sys, k, degree, jacobi):
    """Column groups of 2 (k = 2, 5), 3 (k = 3, 5, 6, 7) and 4 (k = 4, 7); from k = 4 on the mix is asserted."""
    s = cheb_sys
    want = s.single_solves(k, degree, jacobi)
    X0 = s.X0(degree, jacobi)
    got = s.plan.cg_cheb_multi(s.B[:k], degree, X0=X0[:k], **s.kw(jacobi))
    print(f"k={k} degree={degree} jacobi={jacobi}: iterations {list(got[1])}")
    assert_columns_same_bits(got, want, f"k={k} degree={degree} jacobi={jacobi}")
    if k >= 4:
        assert_the_mix(got[1], f"k={k} degree={degree} jacobi={jacobi}")
    if k == 7:
        assert_columns_same_bits(s.plain_launches.cg_cheb_multi(s.B[:k], degree, X0=X0[:k], **s.kw(jacobi)), want,
                                 f"graphs=2 k={k} degree={degree} jacobi={jacobi}")


def test_wide_cheb_kernels_with_the_polynomial_on_the_val_f32_plan(E, gpu, cheb_sys):
    """k = 5: passes of width 1 on the polynomial's plan beside passes of width 4 and 1 on the plan"""
    s, k = cheb_sys, 5
    want = s.single_solves(k, DEGREE, True, f32=True)
    got = s.plan.cg_cheb_multi(s.B[:k], DEGREE, X0=s.X0(DEGREE, True)[:k], **s.kw(True, f32=True))
    print(f"val_f32 polynomial k={k}: iterations {list(got[1])}")
    assert_columns_same_bits(got, want, "val_f32 polynomial, k=5")
    assert_the_mix(got[1], "val_f32 polynomial, k=5")
    # the rounded polynomial is another preconditioner: the iterates differ from those of the fp64 polynomial
    assert not np.array_equal(want[0][2], s.single_solves(k, DEGREE, True)[0][2])


@pytest.mark.parametrize("degree", [0, 1])
def test_degrees_zero_and_one_at_k_5(E, gpu, cheb_sys, degree):
    """degree 0: the start kernel writes the r.z partials; degree 1: the one step kernel has w_in = r and writes them"""
    s, k = cheb_sys, 5
    X0 = s.X0(degree, True)
    want = s.single_solves(k, degree, True)
    got = s.plan.cg_cheb_multi(s.B[:k], degree, X0=X0[:k], **s.kw(True))
    print(f"degree={degree} k={k}: iterations {list(got[1])}")
    assert_columns_same_bits(got, want, f"degree={degree} k=5")
    assert_the_mix(got[1], f"degree={degree} k=5")
    if degree == 0:
        # (lmin, lmax) = (0.5, 1.5): c0 = 1, z = D^-1 r -- ehyb_pcg's preconditioner (test_degree_zero_is_scaled_jacobi)
        want = s.single_solves(k, 0, True, lmin=0.5, lmax=1.5)
        got = s.plan.cg_cheb_multi(s.B[:k], 0, X0=X0[:k], **s.kw(True, lmin=0.5, lmax=1.5))
        assert_columns_same_bits(got, want, "degree=0 (0.5, 1.5) k=5")
        assert_the_mix(got[1], "degree=0 (0.5, 1.5) k=5")
        for j in range(k):
            xj, itj, relj = s.plan.cg(s.B[j], x0=X0[j], max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY, inv_diag=s.inv_diag)
            assert abs(int(got[1][j]) - itj) <= 1, (j, got[1][j], itj)
            assert np.linalg.norm(got[0][j] - xj) <= 1e-9 * np.linalg.norm(xj), j


@pytest.mark.parametrize("k", [5, 7])
def test_wide_cheb_kernels_at_full_size_with_ldb_and_ldx(E, gpu, cheb_sys, k):
    """Q = A X0 reads X at ldx, the init kernel B at ldb, the update kernel writes X at ldx: X0 != 0 in four columns"""
    s, n = cheb_sys, cheb_sys.n
    ldb, ldx = n + 37, n + 5
    X0 = s.X0(DEGREE, True)
    assert sum(bool(X0[j].any()) for j in range(k)) >= 3
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = s.B[:k]
    Xb = np.full((k, ldx), SENTINEL)
    Xb[:, :n] = X0[:k]
    db, dx, dd = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel()), E.DeviceBuffer(n).upload(s.inv_diag)
    it, rel = (C.c_int * k)(), (C.c_double * k)()
    lib = E.host._lib.load()
    rc = lib.ehyb_pcg_cheb_multi(s.plan.h, None, C.c_void_p(dd.ptr), C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, DEGREE, 0.0, LMAX_JACOBI,
                                 MIX_ITERS, MIX_RTOL, MIX_EVERY, None, it, rel)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(Xo[:, n:].view(np.int64), Xb[:, n:].view(np.int64)), "the gap behind the columns of X"
    assert np.array_equal(db.download().view(np.int64), Bb.ravel().view(np.int64))
    assert_columns_same_bits((Xo[:, :n], np.array(list(it)), np.array(list(rel))), s.single_solves(k, DEGREE, True), f"ldb, ldx > n, k={k}")
    assert_the_mix(list(it), f"ldb, ldx > n, k={k}")
    db.free(), dx.free(), dd.free()


def test_a_callers_stream(E, gpu, cheb_sys):
    s, k = cheb_sys, 5
    X0 = s.X0(DEGREE, True)
    ref = s.plan.cg_cheb_multi(s.B[:k], DEGREE, X0=X0[:k], **s.kw(True))
    st = E.Stream()
    try:
        got = s.plan.cg_cheb_multi(s.B[:k], DEGREE, X0=X0[:k], stream=st.ptr, **s.kw(True))
    finally:
        st.destroy()
    assert_columns_same_bits(got, ref, "a caller's stream, k=5")
    assert_columns_same_bits(got, s.single_solves(k, DEGREE, True), "a caller's stream against the single solves")
    assert_the_mix(got[1], "a caller's stream")


# ------------------------------------------------------------------ the solve is the composition of the tested kernels
def composed_cheb(E, s, poly, b, inv_diag, degree, lmin, lmax, L):
    """m -> (x, m, relative residual) for m in COMPOSED_M: ehyb_pcg_cheb's loop written out with ehyb_spmv, the CG step entry
    points (no preconditioner in them: dinv = None) and the two Chebyshev ones; the coefficients through the C ABI"""
    lib, n, plan = E.host._lib.load(), s.n, s.plan
    c0, ca, cb = E.cheb_coeffs(lmin, lmax, degree)
    d = {k: device(E, np.full(n, SENTINEL)) for k in ("r", "p", "q")}
    d["b"], d["x"], d["slots"] = device(E, b), device(E, np.zeros(n)), device(E, np.full(L["slots"] * MAX_GRID, SENTINEL))
    keep = device(E, inv_diag) if inv_diag is not None else None
    dinv = C.c_void_p(keep.ptr) if keep is not None else None
    P = {k: C.c_void_p(v.ptr) for k, v in d.items()}

    def precondition(rz):
        """z = M^-1 r, the partials of r.z into r.z slot number rz"""
        assert lib.ehyb_cheb_start_step(n, P["r"], dinv, c0, P["d"], P["z"], P["slots"], rz if degree == 0 else -1, None) == 0
        for j in range(1, degree + 1):
            poly.spmv(d["d"].ptr, d["q"].ptr)
            assert lib.ehyb_cheb_step(n, P["r" if j == 1 else "w"], P["q"], dinv, float(ca[j - 1]), float(cb[j - 1]), P["w"], P["d"], P["z"], P["r"],
                                      P["slots"], rz if j == degree else -1, None) == 0

    plan.spmv(d["x"].ptr, d["q"].ptr)
    assert lib.ehyb_cg_init_step(n, P["b"], P["q"], None, P["r"], P["p"], P["slots"], None) == 0
    for k in ("d", "z", "w"):
        d[k] = device(E, np.zeros(n))
        P[k] = C.c_void_p(d[k].ptr)
    precondition(0)
    assert lib.ehyb_dev_sync() == 0
    d["p"].upload(d["z"].download())
    out = {}
    for it in range(max(COMPOSED_M)):
        cur = it & 1
        plan.spmv(d["p"].ptr, d["q"].ptr)
        assert lib.ehyb_cg_dot_step(n, P["p"], P["q"], P["slots"], None) == 0
        assert lib.ehyb_cg_update_step(n, P["p"], P["q"], None, P["x"], P["r"], P["slots"], cur, None) == 0
        precondition(cur ^ 1)
        assert lib.ehyb_cg_direction_step(n, P["z"], None, P["p"], P["slots"], cur, None) == 0
        if it + 1 in COMPOSED_M:
            assert lib.ehyb_dev_sync() == 0
            sl = d["slots"].download().reshape(L["slots"], MAX_GRID)
            bb = sc.in_order_sum(sl[L["bb"]])
            out[it + 1] = (d["x"].download(), it + 1, math.sqrt(sc.in_order_sum(sl[L["rr"]]) / (bb if bb > 0 else 1.0)))
    for v in d.values():
        v.free()
    return out


COMPOSED = [(0, False, False), (0, True, False), (1, False, False), (1, True, False), (DEGREE, False, False), (DEGREE, True, False),
            (DEGREE, True, True)]


@pytest.mark.parametrize("degree,jacobi,f32", COMPOSED,
                         ids=[f"degree{d}-{'jacobi' if j else 'plain'}{'-val-f32-polynomial' if f else ''}" for d, j, f in COMPOSED])
def test_pcg_cheb_is_the_composition_of_its_kernels(E, gpu, cheb_sys, cg_layout, degree, jacobi, f32):  # noqa: F811
    s = cheb_sys
    b = s.B[2]                                   # the random right-hand side
    inv = s.inv_diag if jacobi else None
    lmax = LMAX_JACOBI if jacobi else s.lmax_plain
    poly = s.f32 if f32 else s.plan
    want = composed_cheb(E, s, poly, b, inv, degree, lmax / 30.0, lmax, cg_layout)
    for m in COMPOSED_M:
        assert want[m][1] == m and 0 < want[m][2] < np.inf
        for name, plan in (("graph replay", s.plan), ("graphs=2", s.plain_launches)):
            for check_every in (1, 4):
                got = plan.cg_cheb(b, degree, poly_plan=s.f32 if f32 else None, lmax=lmax, max_iter=m, rtol=NEVER, check_every=check_every,
                                   inv_diag=inv)
                assert_solve_same_bits(got, want[m], f"ehyb_pcg_cheb degree={degree} m={m} {name} check_every={check_every} jacobi={jacobi} f32={f32}")


# ------------------------------------------------------------------ the estimate
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_lambda_max_at_full_size(E, gpu, cheb_sys, jacobi):
    """Seven or eight trips of the lambda kernels' grid-stride loop per thread.  1e-9: the bound of
    test_lambda_max_is_a_lower_estimate; Gershgorin's bound stands in for the eigenvalue no one computes at this size."""
    s = cheb_sys
    A = s.s.A
    dinv = 1.0 / A.diagonal() if jacobi else None
    lam = s.plan.lambda_max(s.inv_diag if jacobi else None, 20)
    v0 = E.vector_recover(cc.start_vector(s.n), s.s.perm)
    cpu = cc.lambda_max(A, dinv, 20, v0)
    gershgorin = float((s.rowsum * dinv).max()) if jacobi else float(s.rowsum.max())
    print(f"lambda_max jacobi={jacobi}: device {lam!r}, restatement {cpu!r}, Gershgorin {gershgorin!r}")
    assert abs(lam - cpu) <= 1e-9 * cpu
    assert 0 < lam <= gershgorin
    again = s.plan.lambda_max(s.inv_diag if jacobi else None, 20)
    assert np.array_equal(np.array([lam]).view(np.int64), np.array([again]).view(np.int64))
