"""ehyb_gmres_t: ehyb_gmres for the adjoint system A^T x = b on the plan of A, every multiply an ehyb_spmv_t.

The shapes, matrices, right-hand side and criteria are those of test_gpu_gmres.py, with A replaced by A.T in the references only
(cpu_gmres, the true residual, scipy's direct solve): the plan is built from A.  The transposed multiply adds with atomics, so
nothing here is compared bit for bit.  The shapes the transposed multiply does not serve -- a residual in panel form, symmetric
pair storage -- must be refused before any launch."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from test_gpu_gmres import ERR_ARG, RTOL, SHAPES, System, cpu_gmres, panel_matrix, rhs

pytestmark = pytest.mark.gpu

SERVED = ["halo-window", "reference-window-csr-residual", "direct"]
REFUSED = {"panel-residual": "panel form", "symmetric-pairs": "symmetric pair storage"}
NO_FORWARD_LAUNCH = dict(window=set(), panel=set(), er_csr=set())


def test_the_shapes_are_those_of_test_gpu_gmres():
    assert [s[0] for s in SHAPES] == SERVED + list(REFUSED)


@pytest.mark.parametrize("name,make,taken", [s for s in SHAPES if s[0] in SERVED], ids=SERVED)
def test_plan_shapes_against_cpu_and_scipy(E, gpu, name, make, taken):
    A, kw = make(E)
    At = A.T.tocsr()
    assert abs(A - At).nnz > 0, "the system must be unsymmetric"
    s = System(E, A, **kw)
    assert taken(s.plan.stats) and s.plan.spmv_t_supported, (name, s.plan.stats)
    b = rhs(s.n)
    bp = E.vector_reorder(b, s.perm)
    x_ref = spla.spsolve(At.tocsc(), b)
    x_fwd = E.vector_recover(s.plan.gmres(bp, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)[0], s.perm)
    for restart in (30, 20):
        s.plan.launched_clear()
        xp, it, rel = s.plan.gmres_t(bp, restart=restart, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
        x = E.vector_recover(xp, s.perm)
        _, it_cpu, rel_cpu, status = cpu_gmres(At, b, restart=restart, max_iter=2000, rtol=RTOL, dinv=1.0 / A.diagonal())
        print(name, restart, "device", it, rel, "cpu", it_cpu, rel_cpu, status)
        assert 0 < it and rel <= RTOL, (name, restart, it, rel)
        assert np.linalg.norm(b - At @ x) <= 10 * RTOL * np.linalg.norm(b), (name, restart)
        assert status == "converged" and abs(it - it_cpu) <= 5, (name, restart, it, it_cpu, rel, rel_cpu)
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref), (name, restart, np.linalg.norm(x - x_ref))
        # the adjoint system's solution, not the forward one's; and no forward kernel ran
        assert np.linalg.norm(x - x_fwd) > 1e-3 * np.linalg.norm(x_ref), (name, restart)
        assert s.plan.launched_t() and s.plan.launched() == NO_FORWARD_LAUNCH, (name, s.plan.launched())


@pytest.mark.parametrize("name,make,taken", [s for s in SHAPES if s[0] in REFUSED], ids=list(REFUSED))
def test_unserved_shapes_are_refused_before_any_launch(E, gpu, name, make, taken):
    A, kw = make(E)
    if A is None:
        A = panel_matrix(E, E.make_config(**kw))
    s = System(E, A, **kw)
    assert taken(s.plan.stats) and not s.plan.spmv_t_supported, (name, s.plan.stats)
    bp = E.vector_reorder(rhs(s.n), s.perm)
    s.plan.launched_clear()
    with pytest.raises(E.EhybError) as ei:
        s.plan.gmres_t(bp, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
    assert ei.value.code == ERR_ARG and REFUSED[name] in str(ei.value) and "breakdown" not in str(ei.value), str(ei.value)
    assert s.plan.launched_t() == set() and s.plan.launched() == NO_FORWARD_LAUNCH
    # the forward solver still takes the shape
    x, it, rel = s.plan.gmres(bp, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
    assert 0 < it and rel <= RTOL, (name, it, rel)


def test_null_outputs_max_iter_and_a_user_stream(E, gpu):
    import ctypes as C

    A, kw = SHAPES[0][1](E)
    s = System(E, A, **kw)
    bp = E.vector_reorder(rhs(s.n), s.perm)
    _, it, rel = s.plan.gmres_t(bp, restart=7, max_iter=20, rtol=1e-30, inv_diag=s.inv_diag)      # two graph cycles and a partial one
    assert it == 20 and 0 < rel < 1, (it, rel)
    x, it, rel = s.plan.gmres_t(bp, max_iter=0, rtol=1e-30)
    assert it == 0 and rel == 1.0 and not x.any(), (it, rel)
    st = E.Stream()
    try:
        x, it, rel = s.plan.gmres_t(bp, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag, stream=st.ptr)
    finally:
        st.destroy()
    assert 0 < it < 2000 and rel <= RTOL
    b = E.vector_recover(bp, s.perm)
    assert np.linalg.norm(b - A.T @ E.vector_recover(x, s.perm)) <= 10 * RTOL * np.linalg.norm(b)
    db, dx = E.DeviceBuffer(s.n).upload(bp), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    lib = E.host._lib.load()
    assert lib.ehyb_gmres_t(s.plan.h, None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 30, 2, 1000, RTOL, None, None, None) == 0
    assert np.linalg.norm(b - A.T @ E.vector_recover(dx.download(), s.perm)) <= 10 * RTOL * np.linalg.norm(b)
    assert np.array_equal(db.download(), bp)
