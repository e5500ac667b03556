"""The two kernels of the FSAI preconditioner one launch at a time (ehyb_fsai_factor_step, ehyb_fsai_tt_step).

The factor kernel, one launch per case, on the reordered matrix and the pattern of the library's host object: dense diagonal
blocks of 64 rows, so that the rows of G hold 1, 2, 3, ... 64 columns, at 1, 3, 4, 5, 63, 64, 65 and 1000 rows (a workgroup
takes four rows, one per wave); blocks of 96 rows, so that a row of A is longer than the 64 lanes that walk it, with the
pattern capped at 64 and at 8 columns, below the rows' stored length; and a grid with one indefinite block among good ones.
Every row of g is held to the backward-error bound of fsai_cases.py and compared with the host's row to its forward bound.

The t.t kernel bit for bit on scaled integers (solver_cases.py), with the guards of test_gpu_coarse_kernels.py: every slot entry
that is not written stays, the input comes back unchanged."""
import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as kc
import fsai_cases as fc
from solver_cases import MAX_GRID, SENTINEL, STEP_GRID, Fx, S, odd_ints, partials, walk_profile
from test_gpu_coarse_kernels import Vec, launch
from test_gpu_solver_kernels import cg_layout  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ERR_ARG = 1
WANTED_LENGTHS = {1, 2, 3, 31, 32, 33, 63, 64}


def dense_blocks(n, block, seed):
    """SPD, block diagonal with dense blocks: row i of the lower triangle holds i mod block + 1 entries"""
    rng = np.random.default_rng(seed)
    blocks = []
    for lo in range(0, n, block):
        k = min(block, n - lo)
        M = rng.uniform(-1, 1, (k, k))
        blocks.append(M @ M.T / k + 0.05 * np.eye(k))
    return sp.block_diag(blocks).tocsr()


def factored(E, A, row_cap=0):
    """-> (the reordered matrix as scipy, the host object's row_ptr, cols, vals, the device's g and count of fallback rows)"""
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    f = E.Fsai(m, row_cap=row_cap, cfg=cfg, upload=False)
    row_ptr, cols, vals = f.array("row_ptr"), f.array("cols"), f.array("vals")
    g, fell = E.fsai_factor_step(m.row_idx, m.J, m.V, row_ptr, cols)
    return m.to_scipy(), row_ptr, cols, vals, g, fell, f


def held_to_the_bounds(what, Ap, row_ptr, cols, host, g, skip=()):
    assert np.isfinite(g).all(), f"{what}: a row was not written"
    worst_r, worst_f = fc.rows_within_bounds(Ap, row_ptr, cols, g, other=host, skip=skip)
    print(f"{what}: {len(row_ptr) - 1} rows of up to {np.diff(row_ptr).max()} columns, worst residual / bound {worst_r:.3f}, "
          f"worst distance to the host's row / forward bound {worst_f:.3f}")
    assert worst_r <= 1 and worst_f <= 1


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 1000])
def test_factor_step_row_counts_and_lengths(E, gpu, n):
    Ap, row_ptr, cols, host, g, fell, f = factored(E, dense_blocks(n, 64, n))
    lengths = set(np.diff(row_ptr).tolist())
    assert lengths == set(range(1, min(n, 64) + 1)) and (n < 64 or WANTED_LENGTHS <= lengths)
    assert fell == 0 and f.fallback_rows == 0 and f.capped_rows == 0
    held_to_the_bounds(f"n={n}", Ap, row_ptr, cols, host, g)


@pytest.mark.parametrize("row_cap", [0, 8])
def test_factor_step_long_rows_and_a_capped_pattern(E, gpu, row_cap):
    Ap, row_ptr, cols, host, g, fell, f = factored(E, dense_blocks(192, 96, 7), row_cap)
    stored = np.diff(Ap.indptr)
    assert (stored == 96).all(), "every row of A is longer than the 64 lanes that walk it"
    assert np.diff(row_ptr).max() == (row_cap or 64) and f.capped_rows == 2 * (96 - (row_cap or 64)) and fell == 0
    held_to_the_bounds(f"blocks of 96, row_cap {row_cap}", Ap, row_ptr, cols, host, g)


def test_factor_step_one_indefinite_block_among_good_ones(E, gpu):
    A = kc.near_singular_grid(12, 10, 1, 0.0005).tolil()
    i, j = 5 * 12 + 6, 5 * 12 + 5          # two neighbours in the grid, in no triangle: one block only holds the pair
    A[i, j] = A[j, i] = -10.0 * A[i, i]
    Ap, row_ptr, cols, host, g, fell, f = factored(E, A.tocsr())
    assert fell == 1 and f.fallback_rows == 1
    bad =[r for r in range(len(row_ptr) - 1) if np.linalg.eigvalsh(fc.block(Ap, cols[row_ptr[r]:row_ptr[r + 1]])).min() < 0]
    assert len(bad) == 1
    r = bad[0]
    want = np.zeros(row_ptr[r + 1] - row_ptr[r])
    want[-1] = 1.0 / np.sqrt(Ap[r, r])
    assert len(want) > 1 and np.array_equal(g[row_ptr[r]:row_ptr[r + 1]], want) and np.array_equal(host[row_ptr[r]:row_ptr[r + 1]], want)
    held_to_the_bounds("one indefinite block", Ap, row_ptr, cols, host, g, skip={r})


def test_factor_step_refuses_what_it_cannot_factor(E, gpu):
    A = dense_blocks(5, 64, 1)
    rp, c = fc.pattern(A)[:2]
    with pytest.raises(E.EhybError) as ei:                      # a row of the pattern longer than the dense block
        E.fsai_factor_step(A.indptr, A.indices, A.data, np.array([0, 1, 2, 3, 4, 69]), np.arange(69))
    assert ei.value.code == ERR_ARG and "row 4" in str(ei.value)
    B = A.copy()
    B[2, 2] = -1.0
    with pytest.raises(E.EhybError) as ei:
        E.fsai_factor_step(B.indptr, B.indices, B.data, rp, c)
    assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value)


TT_SIZES = [1, 63, 64, 65, 257, S + 1, 4 * S + 1]


@pytest.mark.parametrize("n", TT_SIZES)
def test_tt_step(E, gpu, cg_layout, n):  # noqa: F811
    L = cg_layout
    profile = walk_profile(n, STEP_GRID)
    assert n != 4 * S + 1 or max(p[0] for p in profile) >= 1, "past the unrolled loop"
    t = Fx(odd_ints(np.random.default_rng(n % 89), n, 13), 3)
    want_tt = partials(t * t, STEP_GRID, "fsai tt")
    for rz in (0, 1):
        tv = Vec(E, n, t.f("t"))
        s = Vec(E, L["slots"] * MAX_GRID, np.full(L["slots"] * MAX_GRID, SENTINEL))
        launch(E, "ehyb_fsai_tt_step", n, tv.ptr, s.ptr, rz)
        want = s.h[:s.n].copy()
        at = (L["rz0"] + 2 * rz) * MAX_GRID
        want[at:at + STEP_GRID] = want_tt.f("tt")
        s.expect(f"tt n={n} rz={rz}: the slots", want)
        tv.expect(f"tt n={n} rz={rz}: t")
