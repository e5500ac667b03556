"""ehyb_pcg_coarse / ehyb_pcg_coarse_multi / ehyb_coarse_apply on the device: two-level PCG against the numpy restatement of
coarse_cases.py, against a direct solve and against ehyb_pcg in the same process.  The hard system is the nearly singular grid
of test_coarse_host.py (plain storage, symmetric pairs, a plan with a CSR residual); then the easy system Jacobi already
suits, a 3-unknowns-per-node pattern with dof = 3, apply alone, reproducibility (runs, graphs against plain launches, a user
stream, check_every), the k-column solve bit for bit against the one-vector one -- also four columns wide at the largest coarse
space, nc = 2048 and 2047, where coarse_solve_kernel<4> asks for all 64 KiB of LDS -- and a coarse object that belongs to another
system.  Everything in the permuted numbering.  (The kernels' unrolled bodies at K > 1: test_gpu_precond_full.py.)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import coarse_cases as kc
from test_gpu_cg import spd_matrix
from test_gpu_cg_multi import assert_same_bits

pytestmark = pytest.mark.gpu

ERR_ARG = 1
RTOL = 1e-10


class System:
    """a reordered matrix, b uniform in [-1, 1] in the permuted numbering, the CPU's numbers (computed once), plans by
    configuration and coarse objects by (agg_rows, dof)"""

    def __init__(self, E, A, **kw):
        self.E, self.kw = E, kw
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(A.indptr, A.indices, A.data, self.cfg, symmetric=True)
        self.m.reorder(self.cfg)
        self.A, self.n = self.m.to_scipy(), self.m.n
        self.b = np.random.default_rng(3).uniform(-1, 1, self.n)
        self.inv_diag = 1.0 / self.A.diagonal()
        self.plans, self.coarses, self.cpu, self.direct = {}, {}, {}, None

    def solved(self):
        """(x* from a sparse direct solve, lambda_min(A) by shift-invert Lanczos) -- computed once, and only for the systems
        whose error is checked: the factors of a grid with random couplings take seconds"""
        if self.direct is None:
            x_star = spla.spsolve(self.A.tocsc(), self.b)
            lam = spla.eigsh(self.A.tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
            self.direct = (x_star, float(lam))
        return self.direct

    def plan(self, **over):
        key = tuple(sorted(over.items()))
        if key not in self.plans:
            self.plans[key] = self.E.Plan(self.m, self.E.make_config(**{**self.kw, **over}))
        return self.plans[key]

    def coarse(self, agg_rows=128, dof=1):
        if (agg_rows, dof) not in self.coarses:
            self.coarses[agg_rows, dof] = self.E.Coarse(self.m, agg_rows=agg_rows, dof=dof)
        return self.coarses[agg_rows, dof]

    def restated(self, agg_rows=128, dof=1):
        """iterations of the restatement's PCG with the library's map (check_every = 1)"""
        if (agg_rows, dof) not in self.cpu:
            co = self.coarse(agg_rows, dof)
            self.cpu[agg_rows, dof] = kc.pcg(self.A, self.b, co.array("map"), co.nc, self.inv_diag, max_iter=5000, rtol=RTOL)[1]
        return self.cpu[agg_rows, dof]

    def check(self, what, x, it, rel, it_cpu):
        """the rules of the hard system: the residual, the error against the direct solve, the iterations against the restatement"""
        x_star, lam_min = self.solved()
        err = np.linalg.norm(x - x_star)
        bound = 2 * RTOL * np.linalg.norm(self.b) / lam_min         # ||e|| <= ||A^-1|| ||r||, ||r|| <= rtol ||b||
        print(f"{what}: {it} iterations, the restatement {it_cpu} (difference {it - it_cpu:+d}); rel {rel:.2e}, "
              f"error {err:.2e} of at most {bound:.2e} (lambda_min {lam_min:.3e})")
        assert rel <= RTOL
        assert err <= bound
        assert abs(it - it_cpu) <= max(2, 0.05 * it_cpu), (it, it_cpu)


@pytest.fixture(scope="module")
def hard(E):
    return System(E, kc.near_singular_grid(120, 100, 1, 0.0005), lds_doubles=2048, sym_pairs=0)


@pytest.fixture(scope="module")
def easy(E):
    return System(E, spd_matrix(120, 100, 3000, 1), lds_doubles=2048, sym_pairs=0)


ARMS = [("plain", dict()), ("symmetric-pairs", dict(sym_pairs=1)), ("csr-residual", dict(window_mode=1, lds_doubles=512))]


@pytest.mark.parametrize("name,plan_kw", ARMS, ids=[a[0] for a in ARMS])
def test_hard_system(E, gpu, hard, name, plan_kw):
    s = hard
    plan, co = s.plan(**plan_kw), s.coarse(128)
    if name == "symmetric-pairs":
        assert plan.stats["sym_pairs"] > 0.25 * s.A.nnz
    if name == "csr-residual":
        assert plan.stats["nnz_er"] > 0
    x, it, rel = plan.cg_coarse(s.b, co, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    _, it_jacobi, rel_jacobi = plan.cg(s.b, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    print(f"{name}: nc = {co.nc}, Jacobi-PCG on the device {it_jacobi} iterations")
    s.check(name, x, it, rel, s.restated(128))
    assert rel_jacobi <= RTOL and 2 * it <= it_jacobi, (it, it_jacobi)


def test_easy_system(E, gpu, easy):
    """diagonally dominant: the coarse space has little to remove, and must not cost iterations (a prototype: 69 against 74)"""
    s = easy
    plan, co = s.plan(), s.coarse(128)
    x, it, rel = plan.cg_coarse(s.b, co, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    _, it_jacobi, rel_jacobi = plan.cg(s.b, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    res = np.linalg.norm(s.A @ x - s.b) / np.linalg.norm(s.b)
    print(f"easy: nc = {co.nc}, {it} iterations, the restatement {s.restated(128)}, Jacobi-PCG on the device {it_jacobi}; rel {rel:.2e}, "
          f"true residual {res:.2e}")
    assert rel <= RTOL and res <= 2 * RTOL and rel_jacobi <= RTOL
    assert it <= it_jacobi + 2, (it, it_jacobi)
    assert abs(it - s.restated(128)) <= max(2, 0.05 * s.restated(128))


def test_three_unknowns_per_node(E, gpu):
    """the pattern of a small fem3d matrix with SPD values, dof = 3 and the automatic agg_rows"""
    pattern = E.Matrix.generate("fem3d", 3000, 3, 10, 10, 13500, 1, 7).to_scipy()
    s = System(E, kc.spd_on_the_pattern(pattern, 0.01), lds_doubles=1024, sym_pairs=0)
    co = s.coarse(0, 3)
    want_map, want_nc = kc.aggregate(s.A.indptr, s.A.indices, s.m.part_boundary, 0, 3, s.m.reorder_list)
    assert co.nc == want_nc and np.array_equal(co.array("map"), want_map) and co.nc > len(s.m.part_boundary) - 1
    x, it, rel = s.plan().cg_coarse(s.b, co, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    s.check(f"fem3d pattern, dof 3, nc = {co.nc}", x, it, rel, s.restated(0, 3))


def test_apply(E, gpu, hard):
    s = hard
    co = s.coarse(128)
    cmap, einv = co.array("map"), co.array("Einv")
    r = np.random.default_rng(11).uniform(-1, 1, s.n)
    for dinv in (s.inv_diag, None):
        z = co.apply(r, dinv)
        want = kc.apply(r, dinv, cmap, einv)
        # relative to the magnitudes of the terms of every entry: |D^-1 r| + (|E^-1| P^T |r|)[map]
        scale = np.abs(r if dinv is None else dinv * r) + (np.abs(einv) @ np.bincount(cmap, weights=np.abs(r), minlength=co.nc))[cmap]
        print(f"apply, inv_diag {dinv is not None}: max error / scale {np.max(np.abs(z - want) / scale):.2e}")
        assert (np.abs(z - want) <= 1e-13 * scale).all()
        assert np.array_equal(z.view(np.int64), co.apply(r, dinv).view(np.int64))


# ------------------------------------------------------------------ reproducibility (plain storage)
def test_runs_graphs_streams_and_check_every_agree_bit_for_bit(E, gpu, hard):
    s = hard
    plan, plain, co = s.plan(), s.plan(graphs=2), s.coarse(128)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2, inv_diag=s.inv_diag)
    st = E.Stream()
    runs = [plan.cg_coarse(s.b, co, **kw), plan.cg_coarse(s.b, co, **kw), plain.cg_coarse(s.b, co, **kw), plan.cg_coarse(s.b, co, stream=st.ptr, **kw)]
    assert runs[0][2] <= RTOL
    for x, it, rel in runs[1:]:
        assert it == runs[0][1] and rel == runs[0][2] and np.array_equal(x.view(np.int64), runs[0][0].view(np.int64))
    # a fixed number of iterations, looked at after every pair or once in eight
    fixed = [p.cg_coarse(s.b, co, rtol=1e-30, max_iter=12, check_every=ce, inv_diag=s.inv_diag) for ce in (1, 8) for p in (plan, plain)]
    for x, it, rel in fixed[1:]:
        assert it == fixed[0][1] == 12 and rel == fixed[0][2] and 0 < rel < 1 and np.array_equal(x.view(np.int64), fixed[0][0].view(np.int64))
    st.destroy()


# ------------------------------------------------------------------ k right-hand sides
def test_multi_is_the_single_solve_column_by_column(E, gpu):
    """k = 5: launches three and two columns wide on a plan whose passes serve four.  A zero b (done at 0 iterations), a nearly
    converged start and random b's: the columns freeze at different check points."""
    s = System(E, kc.near_singular_grid(120, 100, 1, 0.0005), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    plan, co = s.plan(), s.coarse(128)
    assert plan.spmm_max_k == 4 and plan.stats["sym_pairs"] == 0
    assert (plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    rng = np.random.default_rng(5)
    B = np.stack([s.b, np.zeros(s.n), s.b, rng.uniform(-1, 1, s.n), s.A @ rng.uniform(-1, 1, s.n)])
    X0 = np.zeros_like(B)
    X0[2] = s.solved()[0] + 1e-7 * rng.uniform(-1, 1, s.n)
    for inv in (s.inv_diag, None):
        kw = dict(max_iter=5000, rtol=RTOL, check_every=2, inv_diag=inv)
        singles = [plan.cg_coarse(B[j], co, x0=X0[j], **kw) for j in range(5)]
        want = (np.stack([o[0] for o in singles]), np.array([o[1] for o in singles]), np.array([o[2] for o in singles]))
        got = plan.cg_coarse_multi(B, co, X0=X0, **kw)
        print(f"inv_diag {inv is not None}: iterations per column {list(got[1])}")
        assert_same_bits(got, want, f"k=5 inv_diag={inv is not None}")
        assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any()
        assert (got[2] <= RTOL).all() and 0 < got[1][2] < got[1][0] and len(set(got[1].tolist())) >= 3, (got[1], got[2])


# ------------------------------------------------------------------ the widest solve kernel at the largest coarse space
WIDE_RTOL, WIDE_ITERS = 1e-6, 12
# e of the two nearly converged starts (b = A x*, x0 = x* + e u, x* and u uniform in [-1, 1]).  With a map of 2,048 or 2,047
# contiguous runs of five or six rows the restatement (kc.pcg, with inv_diag) has the relative residual of such a start at
# e * (1, 0.114, 0.034, 0.0145) after 0, 2, 4, 6 iterations, so these two cross WIDE_RTOL at check points 4 and 2 (check_every =
# 2), each a factor of 1.8 to 3 from the edges of its interval; the random right-hand sides are between 0.0024 and 0.15 after 12.
WIDE_E = (1.6e-5, 3e-6)


@pytest.fixture(scope="module")
def wide(E):
    """the system of test_multi_is_the_single_solve_column_by_column and a bank of eight columns: random b's, a zero b and two
    nearly converged starts"""
    s = System(E, kc.near_singular_grid(120, 100, 1, 0.0005), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    rng = np.random.default_rng(5)
    x_star = rng.uniform(-1, 1, s.n)
    near = s.A @ x_star
    s.B = np.stack([s.b, np.zeros(s.n), near, rng.uniform(-1, 1, s.n), s.A @ rng.uniform(-1, 1, s.n), near, rng.uniform(-1, 1, s.n),
                    rng.uniform(-1, 1, s.n)])
    s.X0 = np.zeros_like(s.B)
    s.X0[2] = x_star + WIDE_E[0] * rng.uniform(-1, 1, s.n)
    s.X0[5] = x_star + WIDE_E[1] * rng.uniform(-1, 1, s.n)
    return s


@pytest.mark.parametrize("nc", [2048, 2047])
def test_the_widest_solve_kernels_at_the_largest_coarse_space(E, gpu, wide, nc):
    """coarse_solve_kernel<4> stages 4 * ld doubles of dynamic LDS: at nc = EHYB_COARSE_MAX = 2048 exactly 65,536 bytes, and <3>
    49,152.  nc = 2047 has ld = 2048 too: the zero pad column of E^-1 and of the staged T is read.  k = 4, 7 (4 + 3) and 8 (4 + 4)
    against the one-vector solves, whose coarse_solve_kernel<1> test_solve_step of test_gpu_coarse_kernels.py pins exactly at
    these nc; a launch that is refused would leave C = 0 (the loop zeroes it) and other iterates, or an error."""
    s = wide
    plan = s.plan()
    assert plan.spmm_max_k == 4 and plan.stats["sym_pairs"] == 0
    assert (plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    cmap = (np.arange(s.n, dtype=np.int64) * nc // s.n).astype(np.int32)      # contiguous runs of the reordered rows
    co = E.Coarse(s.m, map=cmap)
    row_ptr = co.array("row_ptr")
    assert co.nc == nc and co.array("Einv").shape == (nc, nc) and np.array_equal(co.array("map"), cmap)
    assert len(row_ptr) == nc + 1 and row_ptr[-1] == s.n and (np.diff(row_ptr) >= 1).all()
    kw = dict(max_iter=WIDE_ITERS, rtol=WIDE_RTOL, check_every=2, inv_diag=s.inv_diag)
    singles = [plan.cg_coarse(s.B[j], co, x0=s.X0[j], **kw) for j in range(8)]
    for k in (4, 7, 8):
        want = (np.stack([o[0] for o in singles[:k]]), np.array([o[1] for o in singles[:k]]), np.array([o[2] for o in singles[:k]]))
        got = plan.cg_coarse_multi(s.B[:k], co, X0=s.X0[:k], **kw)
        print(f"nc={nc} k={k}: iterations per column {list(got[1])}, relative residuals {[f'{r:.2e}' for r in got[2]]}")
        assert_same_bits(got, want, f"nc={nc} k={k}")
        assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any()
        assert np.isfinite(got[2]).all() and (got[2] < 1).all(), got[2]
        assert len(set(got[1].tolist())) >= 3, got[1]
    co.destroy()


# ------------------------------------------------------------------ another system's coarse object
def test_a_coarse_object_of_another_system(E, gpu, hard, easy):
    """only a preconditioner: M stays symmetric positive definite, the solve converges; another n is an argument error"""
    assert hard.n == easy.n
    co = hard.coarse(128)
    x, it, rel = easy.plan().cg_coarse(easy.b, co, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=easy.inv_diag)
    print(f"the hard system's coarse object on the easy system: {it} iterations, rel {rel:.2e}")
    assert rel <= RTOL and np.linalg.norm(easy.A @ x - easy.b) <= 2 * RTOL * np.linalg.norm(easy.b)
    off = E.Coarse.raw(easy.n - 1, np.zeros(easy.n - 1, dtype=np.int32), np.ones((1, 1)))
    with pytest.raises(E.EhybError) as ei:
        easy.plan().cg_coarse(easy.b, off, inv_diag=easy.inv_diag)
    assert ei.value.code == ERR_ARG and f"{easy.n - 1} rows" in str(ei.value)
    lib = E.host._lib.load()
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    cold = E.Coarse(easy.m, agg_rows=128, upload=False)
    assert lib.ehyb_pcg_coarse(easy.plan().h, cold.h, None, p, p, 10, 1e-8, 10, None, None, None) == 8 and b"coarse object not uploaded" in lib.ehyb_last_error()
