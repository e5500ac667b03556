"""The two-level and the FSAI solver (ehyb_coarse.hip, ehyb_fsai.hip) at the size where every loop of their kernels runs:
BigSystem of test_gpu_solver_kernels.py, n = 943,104 -- the solve launches 512 workgroups like the *_step entry points, every
thread of coarse_prolong_kernel<K> and fsai_tt_kernel<K> runs the four-stride unrolled body (walk profiles (1,3): one unrolled
trip and three tail trips, and (2,0): two unrolled trips, no tail), and with nc = 1735 unknowns of 6 to 896 rows (half of them
614) a lane of coarse_restrict_kernel<K> makes up to three unrolled trips and then tail ones, and one of coarse_solve_kernel<K>
fourteen trips over K * 13,888 bytes of LDS.  At the 12,000 rows of test_gpu_coarse.py and test_gpu_fsai.py no thread of
prolong or tt enters an unrolled body or makes a second trip; there K = 4 runs on unknowns of five or six rows only
(test_the_widest_solve_kernels_at_the_largest_coarse_space).

  - ehyb_pcg_coarse_multi against ehyb_pcg_coarse and ehyb_pcg_fsai_multi against ehyb_pcg_fsai column by column, k = 2 .. 8:
    launches of <2> (k = 2, 5), <3> (k = 3, 5, 6, 7) and <4> (k = 4, 7, 8) of restrict, solve, prolong and tt, with c0 = 3 behind a
    group of three (k = 5, 6) and c0 = 4 behind a group of four (k = 7: 4 + 3, k = 8: 4 + 4), on a bank whose columns freeze before
    the first iteration, at check points 2, 4 and 6 and never (coarse_cases.MIX_E, fsai_cases.MIX_E; asserted from iters_done),
    so that the flags change between check points inside a group of four while the multiplies keep going over the frozen
    columns; the two-level solver with inv_diag and without (prolong's two branches); G in fp32 (passes of width 1 on G's plans
    beside wide tt launches); ldb > n, ldx > n and X0 != 0 through the C entry points; a caller's stream; plain launches
    (graphs = 2) beside the replayed graph;
  - ehyb_pcg_coarse and ehyb_pcg_fsai as the composition of their own kernels (ehyb_coarse_restrict_step, ehyb_coarse_solve_step,
    ehyb_coarse_prolong_step, ehyb_fsai_tt_step and the CG steps: <1> with active = nullptr, each tested exactly one launch at a
    time in test_gpu_coarse_kernels.py, test_gpu_fsai_kernels.py and test_gpu_solver_kernels.py) and of the multiplies on the
    plans of A, G and G^T: a wrong r.z slot number, parity or set-up order that still converges shows here.

Everything is compared bit for bit (view(np.int64)); no tolerance appears in this file.  transpose="spmv_t" is left out: its
atomic adds arrive in any order."""
import ctypes as C
import math

import numpy as np
import pytest

import cheb_cases as cc
import coarse_cases as kc
import fsai_cases as fc
import solver_cases as sc
from solver_cases import MAX_GRID, SENTINEL
from test_gpu_solver_kernels import (BIG_SPD_KW, COMPOSED_M, MIX_EVERY, MIX_ITERS, MIX_KINDS, MIX_RTOL, NEVER,  # noqa: F401
                                     assert_columns_same_bits, assert_solve_same_bits, assert_the_mix, big_spd, cg_layout, device)

pytestmark = pytest.mark.gpu

ARMS = ("coarse-jacobi", "coarse-plain", "fsai")      # and "fsai-g-f32" in one test
KW = dict(max_iter=MIX_ITERS, rtol=MIX_RTOL, check_every=MIX_EVERY)


class PrecondSystem:
    """big_spd, its coarse object and its FSAI objects, the bank of cheb_cases.mix_bank with an eighth column (one more "near"
    one of the largest e) and the start vectors of coarse_cases.MIX_E and fsai_cases.MIX_E, and the one-vector solves computed
    so far"""

    def __init__(self, E, s):
        self.E, self.s, self.n = E, s, s.n
        self.plan, self.plain_launches, self.inv_diag = s.plan, s.plain_launches, s.inv_diag
        assert self.plan.spmm_max_k == 4
        kinds = list(MIX_KINDS) + [("near", max(e for kind, e in MIX_KINDS if kind == "near"))]
        self.x_star, B, self.U, self.rank = cc.mix_bank(s.A, kinds)
        self.B = np.stack([E.vector_reorder(b, s.perm) for b in B])
        assert len(self.B) == 8 and np.array_equal(self.B[:7].view(np.int64), s.B.view(np.int64)), "the first seven right-hand sides are those of big_spd"
        self.banks, self.singles = {}, {}

        self.co = E.Coarse(s.m, agg_rows=0)
        print(f"the coarse object of the big system: nc = {self.co.nc} (agg_rows {kc.default_agg_rows(self.n)})")
        assert 1 < self.co.nc <= kc.COARSE_MAX

        self.f = E.Fsai(s.m, cfg=s.cfg, transpose="plan")
        self.f32 = E.Fsai(s.m, cfg=E.make_config(val_f32=1, **BIG_SPD_KW), transpose="plan")
        assert all(p.spmm_max_k == 4 for p in self.f.plans) and all(p.spmm_max_k == 1 for p in self.f32.plans)
        for f in (self.f, self.f32):
            assert f.fallback_rows == 0 and f.capped_rows == 0
            for p in f.plans:
                assert p.stats["sym_pairs"] == 0 and (p.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"

    def X0(self, arm):
        es = fc.MIX_E if arm.startswith("fsai") else kc.MIX_E[arm == "coarse-jacobi"]
        if es not in self.banks:
            x0 = cc.mix_x0(self.x_star, self.U, self.rank, es)
            self.banks[es] = np.stack([self.E.vector_reorder(x, self.s.perm) for x in x0])
        return self.banks[es]

    def solve(self, arm, plan, B, X0, stream=0):
        """the k-column solve of B (k, n), or the one-vector solve of B (n,)"""
        multi = "_multi" if B.ndim == 2 else ""
        start = dict(X0=X0) if multi else dict(x0=X0)
        if arm.startswith("coarse"):
            return getattr(plan, "cg_coarse" + multi)(B, self.co, inv_diag=self.inv_diag if arm == "coarse-jacobi" else None, stream=stream, **start, **KW)
        return getattr(plan, "cg_fsai" + multi)(B, self.f32 if arm == "fsai-g-f32" else self.f, stream=stream, **start, **KW)

    def single_solves(self, arm, k):
        X0, out = self.X0(arm), []
        for j in range(k):
            if (arm, j) not in self.singles:
                self.singles[arm, j] = self.solve(arm, self.plan, self.B[j], X0[j])
            out.append(self.singles[arm, j])
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


@pytest.fixture(scope="module")
def precond_sys(E, gpu, big_spd):  # noqa: F811
    return PrecondSystem(E, big_spd)


# ------------------------------------------------------------------ k columns against one
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8])
def test_wide_kernels_at_full_size_equal_the_single_solve(E, gpu, precond_sys, k, arm):
    """Column groups of 2 (k = 2, 5), 3 (k = 3, 5, 6, 7) and 4 (k = 4, 7, 8); c0 = 4 behind a full group at k = 7 and 8; profiles
    (1,3) and (2,0) of prolong's and tt's walk.  From k = 4 on the mix is asserted; at k = 7 the plain launches too."""
    s = precond_sys
    want = s.single_solves(arm, k)
    X0 = s.X0(arm)
    got = s.solve(arm, s.plan, s.B[:k], X0[:k])
    print(f"{arm} k={k}: iterations {list(got[1])}")
    assert_columns_same_bits(got, want, f"{arm} k={k}")
    if k >= 4:
        assert_the_mix(got[1], f"{arm} k={k}")
    if k == 7:
        assert_columns_same_bits(s.solve(arm, s.plain_launches, s.B[:k], X0[:k]), want, f"graphs=2 {arm} k={k}")


def test_wide_fsai_kernels_with_g_in_fp32(E, gpu, precond_sys):
    """k = 5: passes of width 1 on G's plans beside fsai_tt_kernel<3> and <2> and passes of width 4 and 1 on the plan of A"""
    s, k, arm = precond_sys, 5, "fsai-g-f32"
    want = s.single_solves(arm, k)
    got = s.solve(arm, s.plan, s.B[:k], s.X0(arm)[:k])
    print(f"{arm} k={k}: iterations {list(got[1])}")
    assert_columns_same_bits(got, want, f"{arm} k={k}")
    assert_the_mix(got[1], f"{arm} k={k}")
    # the rounded G is another preconditioner: the iterates differ from those of G in fp64
    assert not np.array_equal(want[0][2], s.single_solves("fsai", k)[0][2])


@pytest.mark.parametrize("arm", ["coarse-jacobi", "fsai"])
@pytest.mark.parametrize("k", [5, 7])
def test_wide_kernels_at_full_size_with_ldb_and_ldx(E, gpu, precond_sys, k, arm):
    """Q = A X0 reads X at ldx, the init kernel B at ldb, the update kernel writes X at ldx: X0 != 0 in the near columns; R, Z, T
    and C keep the leading dimensions n and nc"""
    s, n = precond_sys, precond_sys.n
    ldb, ldx = n + 37, n + 5
    X0 = s.X0(arm)
    assert sum(bool(X0[j].any()) for j in range(k)) >= 3
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = s.B[:k]
    Xb = np.full((k, ldx), SENTINEL)
    Xb[:, :n] = X0[:k]
    db, dx, dd = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel()), E.DeviceBuffer(n).upload(s.inv_diag)
    it, rel = (C.c_int * k)(), (C.c_double * k)()
    lib = E.host._lib.load()
    tail = (C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, MIX_ITERS, MIX_RTOL, MIX_EVERY, None, it, rel)
    if arm == "fsai":
        rc = lib.ehyb_pcg_fsai_multi(s.plan.h, s.f.h, *tail)
    else:
        rc = lib.ehyb_pcg_coarse_multi(s.plan.h, s.co.h, C.c_void_p(dd.ptr), *tail)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(Xo[:, n:].view(np.int64), Xb[:, n:].view(np.int64)), "the gap behind the columns of X"
    assert np.array_equal(db.download().view(np.int64), Bb.ravel().view(np.int64))
    assert_columns_same_bits((Xo[:, :n], np.array(list(it)), np.array(list(rel))), s.single_solves(arm, k), f"{arm} ldb, ldx > n, k={k}")
    assert_the_mix(list(it), f"{arm} ldb, ldx > n, k={k}")
    db.free(), dx.free(), dd.free()


@pytest.mark.parametrize("arm", ["coarse-jacobi", "fsai"])
@pytest.mark.parametrize("k", [5, 7])
def test_a_callers_stream(E, gpu, precond_sys, k, arm):
    s = precond_sys
    X0 = s.X0(arm)
    st = E.Stream()
    try:
        got = s.solve(arm, s.plan, s.B[:k], X0[:k], stream=st.ptr)
    finally:
        st.destroy()
    assert_columns_same_bits(got, s.single_solves(arm, k), f"{arm} on a caller's stream, k={k}")
    assert_the_mix(got[1], f"{arm} on a caller's stream, k={k}")


# ------------------------------------------------------------------ the solves are the composition of the tested kernels
def walk_of(index):
    """pcg_loop.h: the walk of multiply number index (0: first to last, 1: last to first; -1 is the set-up's)"""
    return index & 1


def composed_pcg(E, s, b, L, extra, precondition):
    """m -> (x, m, relative residual) for m in COMPOSED_M: the loop of pcg_loop.h written out with ehyb_spmv_walk and the CG step
    entry points (no preconditioner in them: dinv = None).  extra: name -> length of the preconditioner's own vectors (zeroed, as
    z is); precondition(P, d, it, rz) enqueues z = M^-1 r and the partials of r.z into r.z slot number rz, it = -1 at set-up."""
    lib, n, plan = E.host._lib.load(), s.n, s.plan
    d = {k: device(E, np.full(n, SENTINEL)) for k in ("r", "p", "q")}
    d["b"], d["x"], d["slots"] = device(E, b), device(E, np.zeros(n)), device(E, np.full(L["slots"] * MAX_GRID, SENTINEL))
    P = {k: C.c_void_p(v.ptr) for k, v in d.items()}
    plan.spmv(d["x"].ptr, d["q"].ptr, walk=walk_of(-1))
    assert lib.ehyb_cg_init_step(n, P["b"], P["q"], None, P["r"], P["p"], P["slots"], None) == 0
    for name, count in dict(z=n, **extra).items():
        d[name] = device(E, np.zeros(count))
        P[name] = C.c_void_p(d[name].ptr)
    precondition(P, d, -1, 0)
    assert lib.ehyb_dev_sync() == 0
    d["p"].upload(d["z"].download())
    out = {}
    for it in range(max(COMPOSED_M)):
        cur = it & 1
        plan.spmv(d["p"].ptr, d["q"].ptr, walk=walk_of(cur))
        assert lib.ehyb_cg_dot_step(n, P["p"], P["q"], P["slots"], None) == 0
        assert lib.ehyb_cg_update_step(n, P["p"], P["q"], None, P["x"], P["r"], P["slots"], cur, None) == 0
        precondition(P, d, cur, cur ^ 1)
        assert lib.ehyb_cg_direction_step(n, P["z"], None, P["p"], P["slots"], cur, None) == 0
        if it + 1 in COMPOSED_M:
            assert lib.ehyb_dev_sync() == 0
            sl = d["slots"].download().reshape(L["slots"], MAX_GRID)
            bb = sc.in_order_sum(sl[L["bb"]])
            out[it + 1] = (d["x"].download(), it + 1, math.sqrt(sc.in_order_sum(sl[L["rr"]]) / (bb if bb > 0 else 1.0)))
    for v in d.values():
        v.free()
    return out


def composed_coarse(E, s, co, b, inv_diag, L):
    """ehyb_pcg_coarse: restrict -> solve -> prolong between update and direction"""
    lib = E.host._lib.load()
    keep = device(E, inv_diag) if inv_diag is not None else None
    dinv = C.c_void_p(keep.ptr) if keep is not None else None

    def precondition(P, d, it, rz):
        assert lib.ehyb_coarse_restrict_step(co.h, P["r"], P["t"], None) == 0
        assert lib.ehyb_coarse_solve_step(co.h, P["t"], P["c"], None) == 0
        assert lib.ehyb_coarse_prolong_step(co.h, P["r"], dinv, P["c"], P["z"], P["slots"], rz, None) == 0

    out = composed_pcg(E, s, b, L, dict(t=co.nc, c=co.nc), precondition)
    if keep is not None:
        keep.free()
    return out


def composed_fsai(E, s, f, b, L):
    """ehyb_pcg_fsai: t = G r on the plan of G, the partials of t.t, z = G^T t on the plan of G^T, with the walks apply_columns
    gives the two multiplies"""
    lib, n = E.host._lib.load(), s.n
    plan_g, plan_t = f.plans

    def precondition(P, d, it, rz):
        plan_g.spmv(d["r"].ptr, d["t"].ptr, walk=walk_of(it))
        assert lib.ehyb_fsai_tt_step(n, P["t"], P["slots"], rz, None) == 0
        plan_t.spmv(d["t"].ptr, d["z"].ptr, walk=walk_of(it + 1))

    return composed_pcg(E, s, b, L, dict(t=n), precondition)


@pytest.mark.parametrize("arm", ARMS)
def test_pcg_is_the_composition_of_its_kernels(E, gpu, precond_sys, cg_layout, arm):  # noqa: F811
    s = precond_sys
    b = s.B[2]                                   # the random right-hand side
    assert MIX_KINDS[2][0] == "random"
    if arm == "fsai":
        want = composed_fsai(E, s, s.f, b, cg_layout)
    else:
        want = composed_coarse(E, s, s.co, b, s.inv_diag if arm == "coarse-jacobi" else None, cg_layout)
    for m in COMPOSED_M:
        assert want[m][1] == m and 0 < want[m][2] < np.inf
        for name, plan in (("graph replay", s.plan), ("graphs=2", s.plain_launches)):
            for check_every in (1, 4):
                kw = dict(max_iter=m, rtol=NEVER, check_every=check_every)
                if arm == "fsai":
                    got = plan.cg_fsai(b, s.f, **kw)
                else:
                    got = plan.cg_coarse(b, s.co, inv_diag=s.inv_diag if arm == "coarse-jacobi" else None, **kw)
                assert_solve_same_bits(got, want[m], f"{arm} m={m} {name} check_every={check_every}")
