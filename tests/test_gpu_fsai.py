"""ehyb_pcg_fsai / ehyb_pcg_fsai_multi / ehyb_fsai_apply / ehyb_fsai_set_values on the device: FSAI-preconditioned CG against
the numpy restatement of fsai_cases.py, against a direct solve and against ehyb_pcg in the same process, on the two 120 x 100
systems of test_gpu_coarse.py (the nearly singular grid and the diagonally dominant one) with plain storage, symmetric pairs
and a CSR-residual plan for A -- G's plans are always plain.  Then apply alone, the numeric phase repeated on the device (the
same values and new ones, from the host and from device arrays, with an entry order), G in fp32, reproducibility (runs, graphs
against plain launches, a user stream, check_every), k columns bit for bit against the one-vector solves, G^T through
ehyb_spmv_t, and the refusals.  Everything in the permuted numbering.  (fsai_tt_kernel's unrolled body at K > 1:
test_gpu_precond_full.py.)"""
import ctypes as C

import numpy as np
import pytest

import coarse_cases as kc
import fsai_cases as fc
from test_gpu_cg import spd_matrix
from test_gpu_cg_multi import assert_same_bits
from test_gpu_coarse import ARMS, RTOL, System

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
KW = dict(lds_doubles=2048, sym_pairs=0)


class FsaiSystem(System):
    """System with its FSAI objects by (row_cap, transpose, configuration of G's plans) and the restatement's numbers"""

    def __init__(self, E, A, **kw):
        super().__init__(E, A, **kw)
        self.fsais, self.cpu_fsai = {}, {}

    def fsai(self, row_cap=0, transpose="plan", **over):
        key = (row_cap, transpose, tuple(sorted(over.items())))
        if key not in self.fsais:
            self.fsais[key] = self.E.Fsai(self.m, row_cap=row_cap, cfg=self.E.make_config(**{**self.kw, **over}), transpose=transpose)
        return self.fsais[key]

    def G(self, f):
        return fc.matrix(f.array("row_ptr"), f.array("cols"), f.array("vals"))

    def restated_fsai(self, fp32=False):
        """iterations of the restatement's PCG with the library's G (check_every = 1)"""
        if fp32 not in self.cpu_fsai:
            f = self.fsai()
            vals = f.array("vals")
            G = fc.matrix(f.array("row_ptr"), f.array("cols"), vals.astype(np.float32).astype(np.float64) if fp32 else vals)
            self.cpu_fsai[fp32] = fc.pcg(self.A, self.b, G, max_iter=5000, rtol=RTOL)[1]
        return self.cpu_fsai[fp32]


@pytest.fixture(scope="module")
def hard(E):
    return FsaiSystem(E, kc.near_singular_grid(120, 100, 1, 0.0005), **KW)


@pytest.fixture(scope="module")
def easy(E):
    return FsaiSystem(E, spd_matrix(120, 100, 3000, 1), **KW)


@pytest.fixture(params=["hard", "easy"])
def system(request, hard, easy):
    return {"hard": hard, "easy": easy}[request.param]


@pytest.mark.parametrize("name,plan_kw", ARMS, ids=[a[0] for a in ARMS])
def test_solve(E, gpu, system, name, plan_kw):
    s = system
    plan, f = s.plan(**plan_kw), s.fsai()
    if name == "symmetric-pairs":
        assert plan.stats["sym_pairs"] > 0.25 * s.A.nnz
    if name == "csr-residual":
        assert plan.stats["nnz_er"] > 0
    assert all(p.stats["sym_pairs"] == 0 for p in f.plans) and f.fallback_rows == 0 and f.capped_rows == 0
    x, it, rel = plan.cg_fsai(s.b, f, max_iter=5000, rtol=RTOL, check_every=1)
    _, it_jacobi, rel_jacobi = plan.cg(s.b, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    print(f"{name}: Jacobi-PCG on the device {it_jacobi} iterations")
    s.check(name, x, it, rel, s.restated_fsai())
    assert rel_jacobi <= RTOL and 1.5 * it <= it_jacobi, (it, it_jacobi)


def test_apply(E, gpu, system):
    s = system
    f = s.fsai()
    G = s.G(f)
    m_max = int(np.diff(f.array("row_ptr")).max())
    r = np.random.default_rng(11).uniform(-1, 1, s.n)
    z = f.apply(r)
    want = fc.apply(G, r)
    bound = np.abs(abs(G).T @ (abs(G) @ np.abs(r))).max() * 2 * (m_max + 1) * fc.EPS
    print(f"apply: max error {np.abs(z - want).max():.2e} of at most {bound:.2e} (rows of up to {m_max} columns)")
    assert (np.abs(z - want) <= bound).all()
    assert np.array_equal(z.view(np.int64), f.apply(r).view(np.int64))
    zt = s.fsai(transpose="spmv_t").apply(r)
    assert (np.abs(zt - want) <= bound).all()


# ------------------------------------------------------------------ the numeric phase on the device
def test_set_values(E, gpu, system):
    s = system
    plan = s.plan(value_map=1)
    V = s.m.V.copy()
    diag = np.repeat(np.arange(s.n), np.diff(s.m.row_idx)) == s.m.J
    V2 = V.copy()
    V2[diag] *= 1.0 + np.random.default_rng(21).uniform(0, 1, s.n)        # the same pattern, other values, still SPD
    f = E.Fsai(s.m, cfg=s.cfg)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=1)
    it_fresh = s.restated_fsai()

    def solve_and_check(what, want_it, A, V_now):
        x, it, rel = plan.cg_fsai(s.b, f, **kw)
        res = np.linalg.norm(A @ x - s.b) / np.linalg.norm(s.b)
        print(f"{what}: {it} iterations (a fresh object {want_it}), rel {rel:.2e}, true residual {res:.2e}, fallback rows {f.fallback_rows}")
        assert rel <= RTOL and res <= 2 * RTOL and abs(it - want_it) <= 2 and f.fallback_rows == 0

    # the same values, from the host
    f.set_values(V)
    solve_and_check("the same values, host arrays", plan.cg_fsai(s.b, s.fsai(), **kw)[1], s.A, V)
    # a second set: a fresh object built on the host from them is the yardstick
    A2 = s.A.copy()
    A2.data[:] = V2
    s.m.V[:] = V2
    try:
        fresh = E.Fsai(s.m, cfg=s.cfg)
    finally:
        s.m.V[:] = V
    plan.set_values(V2)
    try:
        it2 = plan.cg_fsai(s.b, fresh, **kw)[1]
        f.set_values(V2)
        solve_and_check("new values, host arrays", it2, A2, V2)
        f.set_values(V)                                                     # (and back, so that the next call has something to change)
        order = np.random.default_rng(22).permutation(len(V2)).astype(np.int32)
        shuffled = np.empty_like(V2)
        shuffled[order] = V2                                                # entry k of the reordered matrix sits at order[k]
        padded = np.zeros(len(order) + (len(order) & 1), dtype=np.int32)   # (a DeviceBuffer holds doubles: two int32 each)
        padded[:len(order)] = order
        dv, do = E.DeviceBuffer(len(V2)).upload(shuffled), E.DeviceBuffer(len(padded) // 2).upload(padded.view(np.float64))
        f.set_values((dv.ptr, len(V2)), (do.ptr, len(order)))
        solve_and_check("new values, device arrays with an entry order", it2, A2, V2)
        # an entry order out of range, a diagonal that is not positive: refused, the plans untouched
        bad = order.copy()
        bad[5] = len(V2)
        with pytest.raises(E.EhybError) as ei:
            f.set_values(shuffled, bad)
        assert ei.value.code == ERR_ARG and "entry_order" in str(ei.value)
        V3 = V2.copy()
        V3[np.flatnonzero(diag)[7]] = -1.0
        with pytest.raises(E.EhybError) as ei:
            f.set_values(V3)
        assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value)
        solve_and_check("after two refused calls", it2, A2, V2)
    finally:
        plan.set_values(V)
    assert it_fresh == s.restated_fsai()
    f.destroy()
    fresh.destroy()


def test_fp32_preconditioner(E, gpu, system):
    """G in fp32 on the device (cfg.val_f32 for G's plans), the CG in fp64.  The margin: test_fsai_host.py holds the restatement
    with G rounded to fp32 to a tenth more iterations on both systems (it measures none more), so a tenth it is."""
    s = system
    plan = s.plan()
    f32 = s.fsai(val_f32=1)
    assert all(p.device_value_bytes[0] * 2 == 8 * len(p.array("ell_val")) for p in f32.plans)
    x, it, rel = plan.cg_fsai(s.b, f32, max_iter=5000, rtol=RTOL, check_every=1)
    _, it64, _ = plan.cg_fsai(s.b, s.fsai(), max_iter=5000, rtol=RTOL, check_every=1)
    res = np.linalg.norm(s.A @ x - s.b) / np.linalg.norm(s.b)
    print(f"G in fp32: {it} iterations, in fp64 {it64}; the restatement {s.restated_fsai(True)} and {s.restated_fsai()}; rel {rel:.2e}, true residual {res:.2e}")
    assert s.restated_fsai(True) <= 1.1 * s.restated_fsai()
    assert rel <= RTOL and res <= 2 * RTOL and it <= 1.1 * it64


# ------------------------------------------------------------------ reproducibility (plain storage, transpose="plan")
def test_runs_graphs_streams_and_check_every_agree_bit_for_bit(E, gpu, hard):
    s = hard
    plan, plain, f = s.plan(), s.plan(graphs=2), s.fsai()
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2)
    st = E.Stream()
    runs = [plan.cg_fsai(s.b, f, **kw), plan.cg_fsai(s.b, f, **kw), plain.cg_fsai(s.b, f, **kw), plan.cg_fsai(s.b, f, stream=st.ptr, **kw)]
    assert runs[0][2] <= RTOL
    for x, it, rel in runs[1:]:
        assert it == runs[0][1] and rel == runs[0][2] and np.array_equal(x.view(np.int64), runs[0][0].view(np.int64))
    # a fixed number of iterations, looked at after every one or once in seven
    fixed = [p.cg_fsai(s.b, f, rtol=1e-30, max_iter=14, check_every=ce) for ce in (1, 7) for p in (plan, plain)]
    for x, it, rel in fixed[1:]:
        assert it == fixed[0][1] == 14 and rel == fixed[0][2] and 0 < rel < 1 and np.array_equal(x.view(np.int64), fixed[0][0].view(np.int64))
    st.destroy()


def test_multi_is_the_single_solve_column_by_column(E, gpu):
    """k = 5: tt launches three and two columns wide on plans whose passes serve four columns, A's and G's.  The bank of
    test_gpu_coarse.py's test of the same name -- a zero b (done at 0 iterations), a nearly converged start and random b's: the
    columns freeze at different check points, so the flags change while the solve runs."""
    s = FsaiSystem(E, kc.near_singular_grid(120, 100, 1, 0.0005), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    plan, f = s.plan(), s.fsai()
    assert plan.spmm_max_k == 4 and all(p.spmm_max_k == 4 for p in f.plans)
    for p in (plan,) + f.plans:
        assert (p.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    rng = np.random.default_rng(5)
    B = np.stack([s.b, np.zeros(s.n), s.b, rng.uniform(-1, 1, s.n), s.A @ rng.uniform(-1, 1, s.n)])
    X0 = np.zeros_like(B)
    X0[2] = s.solved()[0] + 1e-7 * rng.uniform(-1, 1, s.n)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2)
    singles = [plan.cg_fsai(B[j], f, x0=X0[j], **kw) for j in range(5)]
    want = (np.stack([o[0] for o in singles]), np.array([o[1] for o in singles]), np.array([o[2] for o in singles]))
    got = plan.cg_fsai_multi(B, f, X0=X0, **kw)
    print(f"iterations per column {list(got[1])}")
    assert_same_bits(got, want, "k=5")
    assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any() and (got[2] <= RTOL).all()
    assert 0 < got[1][2] < got[1][0] and len(set(got[1].tolist())) >= 3, (got[1], got[2])
    # G in fp32: passes of width 1 on G's plans, still the single solves
    f32 = s.fsai(val_f32=1)
    assert all(p.spmm_max_k == 1 for p in f32.plans)
    singles = [plan.cg_fsai(B[j], f32, **kw) for j in (0, 3)]
    got = plan.cg_fsai_multi(B[[0, 3]], f32, **kw)
    assert_same_bits(got, (np.stack([o[0] for o in singles]), np.array([o[1] for o in singles]), np.array([o[2] for o in singles])), "k=2, G in fp32")


# ------------------------------------------------------------------ G^T through ehyb_spmv_t
def test_transpose_by_spmv_t(E, gpu, system):
    """one plan, the order of ehyb_spmv_t's atomic adds: the iteration rule and the residual, no bit claims"""
    s = system
    plan, f = s.plan(), s.fsai(transpose="spmv_t")
    assert f.plans[1] is None
    x, it, rel = plan.cg_fsai(s.b, f, max_iter=5000, rtol=RTOL, check_every=1)
    s.check("spmv_t", x, it, rel, s.restated_fsai())
    B = np.stack([s.b, np.random.default_rng(6).uniform(-1, 1, s.n)])
    X, its, rels = plan.cg_fsai_multi(B, f, max_iter=5000, rtol=RTOL, check_every=1)
    assert (rels <= RTOL).all() and abs(int(its[0]) - s.restated_fsai()) <= max(2, 0.05 * s.restated_fsai())
    assert np.linalg.norm(s.A @ X[1] - B[1]) <= 2 * RTOL * np.linalg.norm(B[1])


# ------------------------------------------------------------------ refusals
def test_refusals(E, gpu, hard):
    s = hard
    lib = E.host._lib.load()
    small = FsaiSystem(E, kc.near_singular_grid(12, 10, 1, 0.0005), **KW)
    with pytest.raises(E.EhybError) as ei:
        s.plan().cg_fsai(s.b, small.fsai())
    assert ei.value.code == ERR_ARG and f"{small.n} rows" in str(ei.value)
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    cold = E.Fsai(s.m, cfg=s.cfg, upload=False)
    assert lib.ehyb_pcg_fsai(s.plan().h, cold.h, p, p, 10, 1e-8, 10, None, None, None) == ERR_STATE and b"fsai object not uploaded" in lib.ehyb_last_error()
    with pytest.raises(E.EhybError) as ei:
        E.Fsai(s.m, cfg=E.make_config(val_f32=1, **KW), transpose="spmv_t")
    refusal = E.Plan(s.m, E.make_config(val_f32=1, **KW), upload=False).spmv_t_refusal
    assert ei.value.code == ERR_ARG == refusal[0] and "val_f32" in refusal[1] and refusal[1] in str(ei.value)
