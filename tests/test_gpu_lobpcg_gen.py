"""ehyb_lobpcg_gen: the smallest modes of K x = lambda M x on the device, M a consistent mass (a plan on K's partitions, through
Matrix.reorder_like) or a lumped one (a diagonal).

K goes through Matrix.from_csr + reorder, M through reorder_like, the lumped mass through vector_reorder.  The start block is a
hash of the row index, so every run here passes X0 = start_block of the ORIGINAL numbering, permuted: the device run is then the
run of the restatement in the original numbering up to the order of sums, and the counts found there carry over.  The restatement
lobpcg_gen_cases.cpu_lobpcg_gen runs on the reordered matrices with the same X0 and the true preconditioner.  For every converging
case, with nrm = max(bnorm max |theta|, anorm):
    nconv == nev
    ||K x_i - theta_i M x_i||_2 <= 10 tol nrm   computed on the host from the returned vectors
    |theta_i - lambda_i|        <= 10 tol nrm   against scipy.linalg.eigh(K, M) (n <= 2000) or eigsh(K, M=M, sigma) with the shift
                                                one below a Gershgorin bound of the pencil (the planted matrix is indefinite)
    max |X M X^T - I|           <= 1e-12
    iters_done                  in [min - 1, max + 1] of count_spread_gen, where the restatement's spread is <= 2 (asserted too)
Iterations / multiplies of the restatement on the REORDERED matrices (its spread of iterations over the plain run and five noisy
runs), consistent | lumped.  In the original numbering the counts are within one or two of these (24, 25, 43, 36; 35, 33, 47, 47;
50, 53, 56, 53): a permutation changes the order of every sum.
    8 x 6 sym_grid(8, 6, 2), nev = nb = 3, tol 1e-10     25 / 75 (25..25) | 26 / 76 (26..26); Jacobi 45 / 133 (45..45) | 38 / 113 (38..38)
    block_diag(B, B), B = sym_grid(30, 20, 5), nev 6,     36 / 257 (35..36) | 35 / 251 (34..35); Jacobi 49 / 386 (48..49) | 48 / 366 (48..49)
      nb 8, tol 1e-10
    planted 120 x 100, nev = nb = 4, tol 1e-10            50 / 145 (50..55) | 51 / 148 (50..52); Jacobi 58 / 201 (58..59) | 59 / 183 (55..59)
    lap_grid(120, 100, 1), Coarse(agg_rows=16),           104 / 332 (103..104)
      consistent, tol 1e-8
    9 x 7 sym_grid(9, 7, 3), nev 1, nb 8, tol 1e-10       19 / 160 (19..19) | 21 / 176 (21..21)
The device on an MI355X, in the order of the rows above: 25 | 26, 45 | 38; 36 | 35, 48 | 49; 51 | 51, 58 | 55; 103; 19 | 21.
Left out of the count assertion, and of no other: on the planted grid the consistent mass without a preconditioner (spread 5 after
reordering) and the lumped mass with Jacobi (spread 4), whose counts move with roundings; the lumped mass without a preconditioner
(spread 8 in the original numbering, 2 after this reordering) runs without it as well.  The tests compute the spreads again and
assert a count only where the spread is <= 2.
Identities, plain storage, exact in bits: a lumped mass of ones with bnorm = 1 is Plan.lobpcg; a mass plan of diag(m) is the lumped
mass m -- for m a power of two at every row: the stored image is rotated, BS Y, where the lumped form scales the rotated S, m o (S Y),
and the two agree to the bit exactly when every product with m is exact --; two runs agree, on a given and a private stream."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigsh_cases as ec
import lobpcg_cases as lc
import lobpcg_gen_cases as lg

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
_dp = C.POINTER(C.c_double)
PLAIN = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
PAIRS = dict(lds_doubles=4096, sym_pairs=1, direct=2)
SMALL = dict(direct=1, sym_pairs=0)
FORMS = ["consistent", "lumped"]


@functools.lru_cache(maxsize=None)
def pencil(name):
    """-> (K, M consistent, lumped) in the original numbering"""
    if name == "planted":
        return (ec.sym_grid(120, 100, 1),) + lg.mass_grid(120, 100, 1)
    if name == "lap":
        return (lc.lap_grid(120, 100, 1),) + lg.mass_grid(120, 100, 1)
    if name == "twice":
        B, (Mb, lb) = ec.sym_grid(30, 20, 5), lg.mass_grid(30, 20, 5)
        return sp.block_diag([B, B]).tocsr(), sp.block_diag([Mb, Mb]).tocsr(), np.concatenate([lb, lb])
    if name == "small":
        return (ec.sym_grid(8, 6, 2),) + lg.mass_grid(8, 6, 2)
    if name == "odd":
        return (ec.sym_grid(9, 7, 3),) + lg.mass_grid(9, 7, 3)
    raise KeyError(name)


class System:
    """K reordered with its plan; M on K's partitions with a plan of its own (mass_kw: its configuration, sym_pairs off); the
    lumped mass permuted; everything the restatement needs in the permuted numbering"""

    def __init__(self, E, K, M, lumped, mass_kw=None, upload=True, **kw):
        self.E, self.n = E, K.shape[0]
        self.cfg = E.make_config(**kw)
        K = K.tocsr()
        self.m = E.Matrix.from_csr(K.indptr, K.indices, K.data, self.cfg, symmetric=False)
        self.m.reorder(self.cfg)
        self.list = self.m.reorder_list.copy()
        self.A = self.m.to_scipy().tocsr()
        self.plan = E.Plan(self.m, self.cfg, upload=upload)
        M = sp.csr_matrix(M)
        self.mm = E.Matrix.from_csr(M.indptr, M.indices, M.data, self.cfg, symmetric=False).reorder_like(self.m)
        self.M = self.mm.to_scipy().tocsr()
        mass_kw = dict(kw, sym_pairs=2) if mass_kw is None else mass_kw
        self.mass_plan = E.Plan(self.mm, E.make_config(**mass_kw), upload=upload)
        self.lumped = E.vector_reorder(lumped, self.list)

    def mass(self, form):
        return self.mass_plan if form == "consistent" else self.lumped

    def host_mass(self, form):
        return self.M if form == "consistent" else self.lumped

    def x0(self, nb):
        return np.array([self.E.vector_reorder(x, self.list) for x in lc.start_block(self.n, nb)])

    def jacobi(self):
        return 1.0 / np.abs(self.A.diagonal())

    def precond(self, inv_diag=None, coarse=None):
        return lc.preconditioner(inv_diag, *((coarse.array("map"), coarse.array("Einv")) if coarse is not None else ()))


def lowest(K, M, nev):
    """the nev lowest eigenvalues of the pencil: dense for n <= 2000, else shift-invert Lanczos at a shift below the spectrum.
    x^T K x >= gK x^T x and gM x^T x <= x^T M x <= GM x^T x (Gershgorin): lambda >= gK / gM where gK < 0, gK / GM otherwise."""
    Md = sp.diags(M) if np.ndim(M) == 1 else M
    if K.shape[0] <= 2000:
        return sla.eigh(K.toarray(), Md.toarray(), eigvals_only=True)[:nev]
    radius = lambda B: np.asarray(abs(B).sum(axis=1)).ravel() - np.abs(B.diagonal())   # noqa: E731
    gK, gM, GM = (K.diagonal() - radius(K)).min(), (Md.diagonal() - radius(Md)).min(), (Md.diagonal() + radius(Md)).max()
    assert gM > 0
    below = gK / (gM if gK < 0 else GM) - 1.0
    return np.sort(spla.eigsh(K.tocsc(), k=nev, M=sp.csc_matrix(Md), sigma=below, which="LM", tol=1e-13)[0])


def check(what, s, form, got, nev, tol, anorm=0.0, bnorm=0.0, spread=None, count=True):
    """the assertions of the module docstring; spread: (min, max, plain info) of count_spread_gen; count=False: the iteration count
    is printed beside the spread and not asserted; count=None: asserted iff the spread is <= 2 -> info"""
    ev, X, info = got
    M = s.host_mass(form)
    Md = sp.diags(M) if np.ndim(M) == 1 else M
    nrm = max((bnorm or 1.0) * np.abs(ev).max(), anorm)
    res = max(np.linalg.norm(s.A @ X[i] - ev[i] * (Md @ X[i])) for i in range(nev))
    err = np.abs(ev - lowest(s.A, M, nev)).max()
    orth = np.abs(X @ (Md @ X.T) - np.eye(nev)).max()
    print(what, "device", info["iters"], info["multiplies"], info["mass_multiplies"], info["nconv"],
          f"res/nrm {res / nrm:.2e} err/nrm {err / nrm:.2e} orth {orth:.1e}",
          "cpu", None if spread is None else (spread[2]["iters"], spread[2]["multiplies"], spread[:2]))
    assert info["nconv"] == nev == len(ev), (what, info)
    assert res <= 10 * tol * nrm, (what, res / nrm)
    assert err <= 10 * tol * nrm, (what, err / nrm)
    assert orth <= 1e-12, (what, orth)
    assert (info["resid"] <= tol * nrm * (1 + 1e-12)).all(), (what, info["resid"])
    assert info["mass_multiplies"] == (info["multiplies"] if form == "consistent" else 0), (what, info)
    if spread is not None:
        lo, hi, plain = spread
        assert plain["status"] == "ok" and plain["nconv"] == nev, (what, plain)
        if count is None:
            count = hi - lo <= 2
            print(what, "count asserted" if count else "count NOT asserted: the restatement's spread exceeds 2", lo, hi)
        if count:
            assert hi - lo <= 2, (what, lo, hi)
            assert lo - 1 <= info["iters"] <= hi + 1, (what, info["iters"], lo, hi)
    return info


def solve(s, form, nev, block=0, jacobi=False, coarse=None, tol=1e-10, count=True, what="", **kw):
    nb = block or nev
    d = s.jacobi() if jacobi or coarse is not None else None
    X0 = s.x0(nb)
    spread = lg.count_spread_gen(s.A, s.host_mass(form), nev, block=block, T=s.precond(d, coarse), X0=X0, tol=tol)
    got = s.plan.lobpcg_gen(nev, s.mass(form), block=block, coarse=coarse, inv_diag=d, X0=X0, tol=tol, **kw)
    return check(f"{what} {form} jacobi={jacobi}", s, form, got, nev, tol, spread=spread, count=count)


# ------------------------------------------------------------------ the converging cases
@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("form", FORMS)
def test_the_8_by_6_grid(E, gpu, form, jacobi):
    solve(System(E, *pencil("small"), **SMALL), form, 3, jacobi=jacobi, what="8x6")


@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("form", FORMS)
def test_a_block_finds_both_copies_of_a_double_eigenvalue(E, gpu, form, jacobi):
    s = System(E, *pencil("twice"), **SMALL)
    solve(s, form, 6, block=8, jacobi=jacobi, what="twice")
    B, Mb, lb = (ec.sym_grid(30, 20, 5),) + lg.mass_grid(30, 20, 5)
    lam = sla.eigh(B.toarray(), Mb.toarray() if form == "consistent" else np.diag(lb), eigvals_only=True)
    ev = s.plan.lobpcg_gen(6, s.mass(form), block=8, X0=s.x0(8), tol=1e-10, vectors=False)[0]
    assert np.abs(ev - np.repeat(lam[:3], 2)).max() <= 10 * 1e-10 * np.abs(ev).max(), "each lambda twice"


@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("form", FORMS)
def test_planted_grid(E, gpu, form, jacobi):
    """lumped without a preconditioner: the restatement's spread is 48 .. 56 in the original numbering -- run without the count
    assertion.  The other three: the count is asserted iff the reordered spread is <= 2 (module docstring)."""
    s = System(E, *pencil("planted"), **PLAIN)
    count = None if jacobi or form == "consistent" else False
    info = solve(s, form, 4, jacobi=jacobi, count=count, what="planted")
    assert info["multiplies"] < 4 + 4 * info["iters"], "soft locking: converged columns leave the active set"


def test_laplacian_grid_with_the_two_level_preconditioner_and_a_consistent_mass(E, gpu):
    s = System(E, *pencil("lap"), **PLAIN)
    coarse = E.Coarse(s.m, agg_rows=16)
    solve(s, "consistent", 4, coarse=coarse, tol=1e-8, count=None, what="lap coarse")


# ------------------------------------------------------------------ the identities, exact in bits
def same_bits(got, want, what, keys=("nconv", "iters", "multiplies")):
    ev, X, info = got
    evw, Xw, infow = want
    assert [info[k] for k in keys] == [infow[k] for k in keys], (what, info, infow)
    assert np.array_equal(ev.view(np.int64), evw.view(np.int64)), (what, ev, evw)
    assert np.array_equal(info["resid"].view(np.int64), infow["resid"].view(np.int64)), (what, info["resid"], infow["resid"])
    assert np.array_equal(X.view(np.int64), Xw.view(np.int64)), (what, np.abs(X - Xw).max())


def test_a_lumped_mass_of_ones_is_lobpcg_bit_for_bit(E, gpu):
    s = System(E, *pencil("planted"), **PLAIN)
    ones, tol = np.ones(s.n), 1e-10
    want = s.plan.lobpcg(4, inv_diag=s.jacobi(), tol=tol)
    assert want[2]["nconv"] == 4 and want[2]["iters"] > 20
    same_bits(s.plan.lobpcg_gen(4, ones, inv_diag=s.jacobi(), tol=tol, bnorm=1.0), want, "planted, Jacobi")
    s = System(E, *pencil("lap"), **PLAIN)
    coarse = E.Coarse(s.m, agg_rows=16)
    want = s.plan.lobpcg(4, coarse=coarse, inv_diag=s.jacobi(), tol=1e-8)
    assert want[2]["nconv"] == 4 and want[2]["iters"] > 20
    same_bits(s.plan.lobpcg_gen(4, ones, coarse=coarse, inv_diag=s.jacobi(), tol=1e-8, bnorm=1.0), want, "lap, coarse")


def test_a_mass_plan_of_a_diagonal_is_the_lumped_mass_bit_for_bit(E, gpu):
    """m = 2^k, k in -2 .. 2 by a hash of the row: see the module docstring"""
    K = pencil("planted")[0]
    n = K.shape[0]
    m = 2.0 ** ((np.arange(n) * 7 + np.arange(n) // 13) % 5 - 2)
    s = System(E, K, sp.diags(m).tocsr(), m, **PLAIN)
    assert np.array_equal(s.M.diagonal(), s.lumped) and s.M.nnz == n
    for jacobi in (False, True):
        run = dict(inv_diag=s.jacobi() if jacobi else None, X0=s.x0(4), tol=1e-10, max_iter=60)
        a, b = s.plan.lobpcg_gen(4, s.mass_plan, **run), s.plan.lobpcg_gen(4, s.lumped, **run)
        assert a[2]["iters"] > 20 and a[2]["mass_multiplies"] == a[2]["multiplies"] and b[2]["mass_multiplies"] == 0
        same_bits(a, b, f"diag(m) as a plan and as a diagonal, jacobi={jacobi}")


@pytest.mark.parametrize("form", FORMS)
def test_plain_storage_is_exact_for_stream_and_run(E, gpu, form):
    s = System(E, *pencil("planted"), **PLAIN)
    run = dict(inv_diag=s.jacobi(), tol=1e-10)
    ref = s.plan.lobpcg_gen(4, s.mass(form), **run)
    assert ref[2]["iters"] >= 30 and ref[2]["nconv"] == 4, ref[2]
    keys = ("nconv", "iters", "multiplies", "mass_multiplies")
    same_bits(s.plan.lobpcg_gen(4, s.mass(form), **run), ref, "second run", keys)
    st = E.Stream()
    try:
        same_bits(s.plan.lobpcg_gen(4, s.mass(form), stream=st.ptr, **run), ref, "user stream", keys)
    finally:
        st.destroy()


# ------------------------------------------------------------------ further
def test_symmetric_pair_storage_of_k_with_a_plain_mass_plan(E, gpu):
    s = System(E, *pencil("planted"), **PAIRS)
    assert s.plan.stats["sym_pairs"] > 0 and s.mass_plan.stats["sym_pairs"] == 0
    got = s.plan.lobpcg_gen(4, s.mass_plan, inv_diag=s.jacobi(), X0=s.x0(4), tol=1e-10)
    check("pairs", s, "consistent", got, 4, 1e-10)


def test_a_four_wide_plan_with_a_default_mass_plan(E, gpu):
    s = System(E, *pencil("planted"), mass_kw=dict(sym_pairs=2), window_mode=2, lds_doubles=20480 // 4, sym_pairs=0)
    assert s.plan.spmm_max_k == 4
    got = s.plan.lobpcg_gen(4, s.mass_plan, inv_diag=s.jacobi(), X0=s.x0(4), tol=1e-10)
    info = check("four-wide", s, "consistent", got, 4, 1e-10)
    assert info["mass_multiplies"] == info["multiplies"] > 4


@pytest.mark.parametrize("form", FORMS)
def test_max_iter_zero_and_exhausted(E, gpu, form):
    s = System(E, *pencil("planted"), **PLAIN)
    M = s.host_mass(form)
    Md = sp.diags(M) if np.ndim(M) == 1 else M
    for max_iter, mult in ((0, 4), (3, 16)):
        ev, X, info = s.plan.lobpcg_gen(4, s.mass(form), max_iter=max_iter, tol=1e-10)
        assert info["iters"] == max_iter and info["multiplies"] == mult and info["nconv"] < 4, info
        assert info["mass_multiplies"] == (mult if form == "consistent" else 0)
        nrm = np.abs(ev).max()
        assert np.abs(X @ (Md @ X.T) - np.eye(4)).max() <= 1e-12 and (np.diff(ev) >= 0).all()
        true = np.array([np.linalg.norm(s.A @ X[i] - ev[i] * (Md @ X[i])) for i in range(4)])
        assert np.abs(true - info["resid"]).max() <= 1e-10 * nrm, "resid is the norm of the residual of the returned pair"
    # a large bnorm, as a large anorm, loosens the test of convergence
    assert s.plan.lobpcg_gen(4, s.mass(form), max_iter=0, bnorm=1e12)[2]["nconv"] == 4
    assert s.plan.lobpcg_gen(4, s.mass(form), max_iter=0, anorm=1e12)[2]["nconv"] == 4


@pytest.mark.parametrize("form", FORMS)
def test_a_block_of_eight_for_one_pair_and_an_odd_n(E, gpu, form):
    s = System(E, *pencil("odd"), **SMALL)
    assert s.n == 63
    X0, tol = s.x0(8), 1e-10
    got = s.plan.lobpcg_gen(1, s.mass(form), block=8, X0=X0, tol=tol)
    check("odd n, nev 1, nb 8", s, form, got, 1, tol,
          spread=lg.count_spread_gen(s.A, s.host_mass(form), 1, block=8, X0=X0, tol=tol), count=None)
    check("odd n, nev 3", s, form, s.plan.lobpcg_gen(3, s.mass(form), X0=s.x0(3), tol=tol), 3, tol)


def test_a_negative_lumped_mass_is_a_breakdown_with_outputs_written(E, gpu):
    s = System(E, *pencil("small"), **SMALL)
    n, ld = s.n, s.n + (s.n & 1)
    bad = s.lumped.copy()
    bad[n // 3] = -1e9
    with pytest.raises(E.EhybError) as ei:
        s.plan.lobpcg_gen(3, bad)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value) and "ehyb_lobpcg_gen" in str(ei.value)
    ev, X, info = s.plan.lobpcg_gen(3, bad, allow_breakdown=True)
    assert info["nconv"] == 0 and info["iters"] == 0 and info["multiplies"] == 3 and info["mass_multiplies"] == 0, info
    assert np.isnan(ev).all() and np.isnan(info["resid"]).all()
    lib = E.host._lib.load()
    pattern = np.arange(3 * ld, dtype=np.float64) * 0.5 - 7.0
    dv, dm = E.DeviceBuffer(len(pattern)).upload(pattern), E.DeviceBuffer(n).upload(bad)
    ints = [C.c_int(-1) for _ in range(4)]
    evals, resid = np.full(3, -3.0), np.full(3, -3.0)
    rc = lib.ehyb_lobpcg_gen(s.plan.h, None, C.c_void_p(dm.ptr), None, None, None, 0, 3, 0, 500, 1e-8, 0.0, 0.0, evals.ctypes.data_as(_dp),
                             C.c_void_p(dv.ptr), ld, None, *(C.byref(i) for i in ints), resid.ctypes.data_as(_dp))
    assert rc == ERR_ARG and b"breakdown" in lib.ehyb_last_error() and b"negative" in lib.ehyb_last_error()
    assert [i.value for i in ints] == [0, 0, 3, 0] and np.isnan(evals).all() and np.isnan(resid).all()
    assert np.array_equal(dv.download().view(np.int64), pattern.view(np.int64)), "evecs_dev stays"


def test_refusals_on_an_uploaded_plan(E, gpu):
    s = System(E, *pencil("small"), **SMALL)
    other = System(E, *pencil("odd"), upload=False, **SMALL)
    lib = E.host._lib.load()
    dm = E.DeviceBuffer(s.n + 2).upload(np.ones(s.n + 2))

    def call(mass_plan, mdiag):
        rc = lib.ehyb_lobpcg_gen(s.plan.h, mass_plan.h if mass_plan is not None else None, C.c_void_p(mdiag) if mdiag else None, None, None,
                                 None, 0, 3, 0, 5, 1e-8, 0.0, 0.0, None, None, 0, None, None, None, None, None, None)
        return rc, lib.ehyb_last_error()

    for mass_plan, mdiag, code, word in ((s.mass_plan, dm.ptr, ERR_ARG, b"exactly one"), (None, 0, ERR_ARG, b"exactly one"),
                                         (other.mass_plan, 0, ERR_ARG, b"63"), (None, dm.ptr + 8, ERR_ARG, b"mass_diag_dev"),
                                         (s.mass_plan, 0, 0, b""), (None, dm.ptr, 0, b"")):
        rc, msg = call(mass_plan, mdiag)
        assert rc == code and word in msg, (rc, msg)
    never = System(E, *pencil("small"), upload=False, **SMALL)
    rc, msg = call(never.mass_plan, 0)
    assert rc == ERR_STATE and b"mass plan not uploaded" in msg, msg
    with pytest.raises(AssertionError):
        s.plan.lobpcg_gen(3, np.ones(s.n + 1))
