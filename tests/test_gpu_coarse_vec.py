"""ehyb_pcg_coarse / ehyb_pcg_coarse_multi / ehyb_coarse_apply / ehyb_lobpcg with a coarse object built from near-null-space
vectors (ehyb_coarse_create_host_vecs), on the device: against the numpy restatement of coarse_vec_cases.py run with the
library's own agg, off, W and E^-1, on the 5,760-row spring network of test_coarse_vec_host.py (six rigid-body modes) and on the
nearly singular grid ([1, x, y]); what the rotations buy on the device; the translations against the plain dof = 3 object;
reproducibility (runs, graphs against plain launches, a user stream, check_every); the k-column solve bit for bit against the
one-vector one; ehyb_lobpcg preconditioned with the modes; and the refusals.  Everything in the permuted numbering, plain
storage."""
import ctypes as C

import numpy as np
import pytest

import coarse_cases as kc
import coarse_vec_cases as vc
from test_coarse_vec_host import Net
from test_gpu_cg_multi import assert_same_bits

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
RTOL = 1e-10
SHIFT = 1e-3


class System(Net):
    """Net with plans by configuration and uploaded vector objects by (columns of B, agg_rows)"""

    def __init__(self, E, A, B):
        super().__init__(E, A, B)
        self.E, self.plans, self.objects = E, {}, {}

    def plan(self, **over):
        key = tuple(sorted(over.items()))
        if key not in self.plans:
            self.plans[key] = self.E.Plan(self.m, self.E.make_config(lds_doubles=2048, sym_pairs=0, **over))
        return self.plans[key]

    def coarse(self, nv, agg_rows=128):
        if (nv, agg_rows) not in self.objects:
            co = self.E.Coarse.from_vectors(self.m, self.B[:nv], agg_rows=agg_rows)
            self.objects[nv, agg_rows] = (co, vc.prolongation(co.array("map"), co.array("off"), co.array("W")), co.array("Einv"))
        return self.objects[nv, agg_rows]


@pytest.fixture(scope="module")
def net(E):
    K, coords = vc.spring_network(16, 12, 10, SHIFT, seed=1)
    return System(E, K, E.rigid_body_modes(coords, 3))


@pytest.fixture(scope="module")
def grid(E):
    nx, ny = 120, 100
    i = np.arange(nx * ny)
    return System(E, kc.near_singular_grid(nx, ny, 1, 0.0005), np.stack([np.ones(nx * ny), (i % nx).astype(float), (i // nx).astype(float)]))


def solve(s, nv, agg_rows=128):
    """-> (iterations on the device, iterations of the restatement)"""
    co, P, einv = s.coarse(nv, agg_rows)
    x, it, rel = s.plan().cg_coarse(s.b, co, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=s.dinv)
    it_cpu = s.restated(co)
    res = np.linalg.norm(s.A @ x - s.b) / np.linalg.norm(s.b)
    print(f"nv={nv} agg_rows={agg_rows}: {co.nagg} aggregates, nc={co.nc}; {it} iterations, the restatement {it_cpu}; rel {rel:.2e}, true {res:.2e}")
    assert rel <= RTOL and res <= 2 * RTOL
    assert abs(it - it_cpu) <= max(2, 0.05 * it_cpu), (it, it_cpu)
    return it, it_cpu


def test_spring_network(E, gpu, net):
    """the six modes converge, count as the restatement counts, and need at most two thirds of what the translations need"""
    for agg_rows in (128, 64):
        it_rbm, _ = solve(net, 6, agg_rows)
        it_tr, _ = solve(net, 3, agg_rows)
        assert 3 * it_rbm <= 2 * it_tr, (agg_rows, it_rbm, it_tr)


def test_grid(E, gpu, grid):
    it_vec, _ = solve(grid, 3)
    it_const, _ = solve(grid, 1)
    assert it_vec < it_const


def apply_scale(r, dinv, P, einv):
    """the magnitudes of the terms of every entry: |D^-1 r| + |P| |E^-1| |P|^T |r|"""
    return np.abs(r if dinv is None else dinv * r) + abs(P) @ (np.abs(einv) @ (abs(P).T @ np.abs(r)))


@pytest.mark.parametrize("which,nv", [("net", 6), ("net", 2), ("grid", 3)])
def test_apply(E, gpu, net, grid, which, nv):
    """Plan-independent: Coarse.apply against the restatement, to 1e-13 of the magnitudes of an entry's terms (the margin of
    test_gpu_coarse.test_apply), and the same bits twice"""
    s = {"net": net, "grid": grid}[which]
    co, P, einv = s.coarse(nv)
    r = np.random.default_rng(11).uniform(-1, 1, s.n)
    for dinv in (s.dinv, None):
        z = co.apply(r, dinv)
        want = vc.apply(r, dinv, P, einv)
        scale = apply_scale(r, dinv, P, einv)
        print(f"{which} nv={nv} inv_diag {dinv is not None}: max error / scale {np.max(np.abs(z - want) / scale):.2e}")
        assert (np.abs(z - want) <= 1e-13 * scale).all()
        assert np.array_equal(z.view(np.int64), co.apply(r, dinv).view(np.int64))


def test_the_translations_are_the_plain_dof_object_on_the_device(E, gpu, net):
    """the margin of test_coarse_vec_host.test_the_translations_are_the_plain_dof_object: 16 cond(E) 2^-52 ||z||"""
    co, _, _ = net.coarse(3)
    plain = E.Coarse(net.m, agg_rows=128, dof=3)
    assert co.nc == plain.nc
    cond = np.linalg.cond(plain.array("E"))
    r = np.random.default_rng(11).uniform(-1, 1, net.n)
    for dinv in (net.dinv, None):
        z, want = co.apply(r, dinv), plain.apply(r, dinv)
        err = np.linalg.norm(z - want) / np.linalg.norm(want)
        print(f"inv_diag {dinv is not None}: ||z_vec - z_plain|| / ||z|| = {err:.2e}, margin {16 * cond * 2.0 ** -52:.2e}")
        assert err <= 16 * cond * 2.0 ** -52


# ------------------------------------------------------------------ reproducibility (plain storage)
def test_runs_graphs_streams_and_check_every_agree_bit_for_bit(E, gpu, net):
    s = net
    plan, plain, (co, _, _) = s.plan(), s.plan(graphs=2), s.coarse(6)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2, inv_diag=s.dinv)
    st = E.Stream()
    runs = [plan.cg_coarse(s.b, co, **kw), plan.cg_coarse(s.b, co, **kw), plain.cg_coarse(s.b, co, **kw), plan.cg_coarse(s.b, co, stream=st.ptr, **kw)]
    assert runs[0][2] <= RTOL
    for x, it, rel in runs[1:]:
        assert it == runs[0][1] and rel == runs[0][2] and np.array_equal(x.view(np.int64), runs[0][0].view(np.int64))
    # a fixed number of iterations, looked at after every one or once in ten
    fixed = [p.cg_coarse(s.b, co, rtol=1e-30, max_iter=20, check_every=ce, inv_diag=s.dinv) for ce in (1, 10) for p in (plan, plain)]
    for x, it, rel in fixed[1:]:
        assert it == fixed[0][1] == 20 and rel == fixed[0][2] and 0 < rel < 1 and np.array_equal(x.view(np.int64), fixed[0][0].view(np.int64))
    st.destroy()


@pytest.mark.parametrize("nv", [6, 5])
def test_multi_is_the_single_solve_column_by_column(E, gpu, net, nv):
    """k = 2, 3, 4: one launch of every width.  A zero b (inactive from the start), random b's and a b in the range of A.  nv = 5
    runs under the bound 6: a column of the bound that no aggregate has."""
    s = net
    plan, (co, _, _) = s.plan(), s.coarse(nv)
    rng = np.random.default_rng(5)
    B = np.stack([s.b, np.zeros(s.n), rng.uniform(-1, 1, s.n), s.A @ rng.uniform(-1, 1, s.n)])
    for inv in (s.dinv, None):
        kw = dict(max_iter=5000, rtol=RTOL, check_every=2, inv_diag=inv)
        singles = [plan.cg_coarse(B[j], co, **kw) for j in range(4)]
        for k in (2, 3, 4):
            want = (np.stack([o[0] for o in singles[:k]]), np.array([o[1] for o in singles[:k]]), np.array([o[2] for o in singles[:k]]))
            got = plan.cg_coarse_multi(B[:k], co, **kw)
            print(f"nv={nv} k={k} inv_diag {inv is not None}: iterations per column {list(got[1])}")
            assert_same_bits(got, want, f"nv={nv} k={k} inv_diag={inv is not None}")
            assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any()
            assert (got[2] <= RTOL).all()


# ------------------------------------------------------------------ the eigensolver through the apply
def test_lobpcg_with_the_modes(E, gpu, net):
    """The six lowest eigenvalues of the spring network are the shift, six times.  The residual test is relative to anorm = the
    largest diagonal entry (a lower bound of ||A||); with the modes in the coarse space the solve takes no more iterations than
    with the plain dof = 3 object."""
    tol, anorm = 1e-8, float(net.A.diagonal().max())
    co, _, _ = net.coarse(6)
    plain = E.Coarse(net.m, agg_rows=128, dof=3)
    out = {}
    for name, c in (("modes", co), ("dof3", plain)):
        ev, X, info = net.plan().lobpcg(6, block=6, coarse=c, inv_diag=net.dinv, tol=tol, anorm=anorm, max_iter=500)
        print(f"{name}: {info['iters']} iterations, {info['multiplies']} multiplies, max |ev - shift| = {np.abs(ev - SHIFT).max():.2e}")
        assert info["nconv"] == 6 and np.abs(ev - SHIFT).max() <= tol * anorm
        assert np.abs(X @ X.T - np.eye(6)).max() <= 1e-10
        out[name] = info["iters"]
    assert out["modes"] <= out["dof3"], out


# ------------------------------------------------------------------ refusals
def test_refusals(E, gpu, net, grid):
    co, _, _ = grid.coarse(3)
    with pytest.raises(E.EhybError) as ei:
        net.plan().cg_coarse(net.b, co, inv_diag=net.dinv)
    assert ei.value.code == ERR_ARG and f"{grid.n} rows" in str(ei.value)
    with pytest.raises(E.EhybError) as ei:
        net.plan().lobpcg(2, coarse=co)
    assert ei.value.code == ERR_ARG and f"{grid.n} rows" in str(ei.value)
    lib = E.host._lib.load()
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    cold = E.Coarse.from_vectors(net.m, net.B, agg_rows=128, upload=False)
    assert lib.ehyb_pcg_coarse(net.plan().h, cold.h, None, p, p, 10, 1e-8, 10, None, None, None) == ERR_STATE
    assert b"coarse object not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_pcg_coarse_multi(net.plan().h, cold.h, None, p, net.n, p, net.n, 2, 10, 1e-8, 10, None, None, None) == ERR_STATE
