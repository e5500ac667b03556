"""Iterative refinement (csrc/ehyb_refine.hip): ehyb_pcg_refine gets fp64 answers from a plan whose values the device holds in
fp32.  First its two vector kernels one launch at a time, bit for bit, on the exact inputs of solver_cases.py (scaled integers,
sentinels behind every vector, every single partial compared) at sizes that cover the unrolled trips and tails of a 512-workgroup
grid; then the solve, on a system whose fp32-rounded form has a solution that is NOT good enough -- asserted on the CPU first."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import solver_cases as sc
from solver_cases import MAX_GRID, S, STEP_GRID
from test_gpu_solver_kernels import Bench
from val_f32_cases import f32

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 4 * S + 1, 943695]
R_RR, R_BB, R_SLOTS = 0, 1, 2           # s[0 .. slot_doubles) = partials of r.r, s[slot_doubles .. 2 slot_doubles) of b.b


@pytest.mark.parametrize("n", SIZES)
def test_refine_residual_step(E, gpu, n):
    """r = b - q with the partials of r.r and b.b: b and r odd 13-bit numbers over 8 (their squares are wide, as in the init
    kernels of the solvers), q = b - r."""
    walk = sc.walk_profile(n, STEP_GRID)
    assert n not in sc.WALK or walk == sc.WALK[n]
    rng = np.random.default_rng(n % 83)
    b, r = sc.Fx(sc.odd_ints(rng, n, 13), 3), sc.Fx(sc.odd_ints(rng, n, 13), 3)
    q = b - r
    bench = Bench(E, n, R_SLOTS).vecs({"b": b, "q": q}).vec("r")
    bench.call("ehyb_refine_residual_step", "b", "q", "r", "slots")
    bench.expect(f"refine residual n={n}", {"r": r}, {R_RR: sc.partials(r * r, STEP_GRID, "r.r"), R_BB: sc.partials(b * b, STEP_GRID, "b.b")})


@pytest.mark.parametrize("n", SIZES)
def test_refine_axpy_step(E, gpu, n):
    """x += d: x odd 26-bit numbers over 4, d odd 25-bit numbers over 32 -- neither fits fp32, nor does the sum"""
    rng = np.random.default_rng(n % 79)
    x, d = sc.Fx(sc.odd_ints(rng, n, 26), 2), sc.Fx(sc.odd_ints(rng, n, 25), 5)
    total = x + d
    assert n == 0 or sc.wide_share(total.m) == 1.0
    bench = Bench(E, n, 1).vecs({"d": d, "x": x})
    bench.call("ehyb_refine_axpy_step", "d", "x")
    bench.expect(f"refine axpy n={n}", {"x": total}, {})


def test_step_sizes_cover_the_walk():
    """the sizes reach a first and a second unrolled trip, every tail count before the first, and tails behind a trip"""
    seen = set().union(*(sc.walk_profile(n, STEP_GRID) for n in SIZES))
    assert {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 3), (2, 0)} <= seen


# ---------------------------------------------------------------------------------------------- the solve
RTOL = 1e-12


@pytest.fixture(scope="module")
def system(E):
    """A strictly diagonally dominant SPD matrix of 12,000 rows with real values (fp32 holds none of them), b, and what the CPU
    says about refinement on it."""
    rng = np.random.default_rng(5)
    nx, ny, extra = 120, 100, 3000
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel(), rng.integers(0, n, extra)])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel(), rng.integers(0, n, extra)])
    keep = r != c
    r, c = r[keep], c[keep]
    v = -(1.0 + 2.0 * rng.random(len(r)))
    A = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() * (1.0 + 0.25 * rng.random(n)) + 0.5)).tocsr()
    A.sort_indices()
    assert (f32(A.data) != A.data).mean() > 0.99 and abs(A - A.T).max() == 0
    b = rng.standard_normal(n)
    nb = np.linalg.norm(b)
    A32 = sp.csr_matrix((f32(A.data), A.indices, A.indptr), shape=A.shape)
    lu32 = spla.splu(A32.tocsc())
    # the exact solution of the rounded system is not a solution of the system: refinement is needed
    miss = np.linalg.norm(b - A @ lu32.solve(b)) / nb
    assert miss > 100 * RTOL, miss
    # the outer loop with a direct inner solve
    x, prev, steps = np.zeros(n), np.inf, 0
    while True:
        res = b - A @ x
        rel = np.linalg.norm(res) / nb
        if rel <= RTOL or not rel <= 0.5 * prev or steps >= 10:
            break
        prev = rel
        x += lu32.solve(res)
        steps += 1
    assert rel <= RTOL and steps <= 5, (rel, steps)
    return dict(A=A, b=b, nb=nb, n=n, cpu_steps=steps, miss=miss)


def _plans(E, sysm, **more):
    kw = dict(window_mode=2, lds_doubles=2048, direct=2, **more)
    cfg1, cfg0 = E.make_config(val_f32=1, **kw), E.make_config(**kw)
    A = sysm["A"]
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg1, symmetric=True)
    m.reorder(cfg1)
    perm = m.reorder_list.copy()
    return m, perm, E.Plan(m, cfg0), E.Plan(m, cfg1), cfg0


@pytest.mark.parametrize("sym_pairs", [0, 1], ids=["plain", "symmetric-pairs"])
def test_pcg_refine_reaches_fp64_accuracy(E, gpu, system, sym_pairs):
    A, b, nb, n = system["A"], system["b"], system["nb"], system["n"]
    m, perm, p64, p32, _ = _plans(E, system, sym_pairs=sym_pairs)
    assert p32.device_value_bytes[0] * 2 == p64.device_value_bytes[0]
    bp, dinv = E.vector_reorder(b, perm), E.vector_reorder(1.0 / A.diagonal(), perm)
    bound = RTOL * nb + 1e-12 * np.linalg.norm(abs(A) @ np.abs(spla.spsolve(A.tocsc(), b)))
    for what, inner in (("fp32 inner plan", p32), ("fp64 inner plan (restarted CG)", p64)):
        xp, outer, inner_its, rel = p64.pcg_refine(inner, bp, max_outer=10, inner_max_iter=500, rtol=RTOL, inner_rtol=1e-6, inv_diag=dinv)
        x = E.vector_recover(xp, perm)
        true = np.linalg.norm(b - A @ x)
        print(f"{what}: {outer} outer steps, {inner_its} inner iterations, reported {rel:.3e}, recomputed {true / nb:.3e} "
              f"(CPU loop with a direct inner solve: {system['cpu_steps']} steps; the rounded system alone misses by {system['miss']:.3e})")
        assert rel <= RTOL, (what, rel)
        assert 1 <= outer <= system["cpu_steps"] + 2 and inner_its >= outer, (what, outer, inner_its)
        assert true <= bound, (what, true, bound)
    # pcg alone on the val_f32 plan solves the ROUNDED system: converged by its own report, and off the true system
    xp, its, rel = p32.cg(bp, max_iter=2000, rtol=RTOL, inv_diag=dinv)
    assert rel <= RTOL and its < 2000
    off = np.linalg.norm(b - A @ E.vector_recover(xp, perm)) / nb
    assert off > 100 * RTOL, off
    p64.destroy(), p32.destroy()


def test_pcg_refine_refuses_plans_that_do_not_fit(E, gpu, system):
    b, n = system["b"], system["n"]
    m, perm, p64, p32, cfg0 = _plans(E, system)
    bp = E.vector_reorder(b, perm)
    # another number of rows
    small = E.Matrix.generate("stencil2d", 50, 50, 5, 0, 1, cfg=cfg0)
    small.reorder(cfg0)
    other = E.Plan(small, cfg0)
    assert other.n != n
    # a plan over some of the rows
    pb = m.part_boundary
    part = E.Plan(m, cfg0, rows=(0, int(pb[len(pb) // 2])))
    never = E.Plan(m, cfg0, upload=False)
    for plan, inner in ((p64, other), (p64, part), (part, p32), (p64, never)):
        with pytest.raises(E.EhybError) as ei:
            plan.pcg_refine(inner, bp)
        assert ei.value.code == (8 if inner is never else 1), ei.value     # EHYB_ERR_ARG; EHYB_ERR_STATE for the plan never uploaded
    for p in (p64, p32, other, part, never):
        p.destroy()
