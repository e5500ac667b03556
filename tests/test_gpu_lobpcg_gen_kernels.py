"""The two kernels of ehyb_lobpcg_gen, each with its fixed-order sum, through ehyb_lobpcg_gram_b_step and ehyb_lobpcg_resid_b_step,
bit for bit, on the inputs of lobpcg_gen_cases.py: every output is one number in fp64 whatever the order of summation, so every
entry is compared exactly.  No tolerance appears in this file.  One launch per case.

Both mass forms: BS (BX) in memory, a third set of integers of its own, and the lumped mass m in {1, 2, 4} applied by the kernel.
Guards as test_gpu_lobpcg_kernels.py: sentinel pads, sentinel rows n .. ld, inputs unchanged; W starts as NaN, and the columns the
mask does not list and the padding row of an odd n must keep it.  The Gram sizes: 1, around one wave of pairs (63, 64, 65) and one
tile of 128 rows (127, 128, 129), several tiles (1000), one row past 32 tiles (4097), and 70001 > 256 workgroups x 128 rows x 2, where
a workgroup walks a third tile.  With BS = S (BX = X), or m = 1, on inputs whose sums round, the outputs must be the bits of
ehyb_lobpcg_gram_step (ehyb_lobpcg_resid_step): the order of every sum is that kernel's."""
import ctypes as C

import numpy as np
import pytest

import lobpcg_cases as lc
import lobpcg_gen_cases as lg
from solver_cases import PAD, SENTINEL
from test_gpu_lobpcg_kernels import RESID_SCRATCH, SCRATCH_DOUBLES, Arrays, columns

pytestmark = pytest.mark.gpu

ERR_ARG = 1
FORMS = [False, True]
FORM_IDS = ["stored", "lumped"]


@pytest.fixture(scope="module")
def scratch(E, gpu):
    return E.DeviceBuffer(SCRATCH_DOUBLES)


def gram_b(lib, a, n, ld, mc, lumped, scratch):
    return lib.ehyb_lobpcg_gram_b_step(n, ld, a.ptr("S"), a.ptr("AS"), a.ptr(None if lumped else "BS"), a.ptr("m" if lumped else None), mc,
                                       a.ptr("G"), a.ptr("H"), C.c_void_p(scratch.ptr), None)


@pytest.mark.parametrize("lumped", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("mc", lg.GRAM_COLS)
@pytest.mark.parametrize("n", lg.GRAM_SIZES)
def test_gram_b_step(E, gpu, scratch, n, mc, lumped):
    """G = S^T BS and H = S^T AS against the int64 products, both triangles; a column more than mc behind S, AS and BS, full of
    sentinels, is not read"""
    lib = E.host._lib.load()
    c = lg.gram_b_case(n, mc, lumped, seed=n % 89 + mc)
    ld = n + (n & 1) + (6 if mc & 1 else 0)
    a = Arrays(E).put("S", columns(c["S"], n, ld, extra=1)).put("AS", columns(c["AS"], n, ld, extra=1))
    if lumped:
        a.put("m", np.concatenate([c["m"], np.full(ld - n, SENTINEL)]))
    else:
        a.put("BS", columns(c["BS"], n, ld, extra=1))
    a.put("G", np.full(mc * mc, SENTINEL)).put("H", np.full(mc * mc, SENTINEL))
    assert gram_b(lib, a, n, ld, mc, lumped, scratch) == 0, lib.ehyb_last_error()
    a.host["G"][:mc * mc] = c["G"].T.ravel()                     # column-major
    a.host["H"][:mc * mc] = c["H"].T.ravel()
    a.expect(f"gram_b n={n} mc={mc} ld={ld} lumped={lumped}")
    G = a.dev["G"].download()[:mc * mc].reshape(mc, mc)
    H = a.dev["H"].download()[:mc * mc].reshape(mc, mc)
    assert np.array_equal(G, G.T) and np.array_equal(H, H.T)


@pytest.mark.parametrize("lumped", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n,mc", [(70001, 24), (4097, 9), (129, 17), (1, 1)])
def test_gram_b_with_the_identity_is_gram_step_bit_for_bit(E, gpu, scratch, n, mc, lumped):
    """normal deviates: every sum rounds at every term, so equal bits mean equal order -- rows per lane, tiles, shuffle tree, grid"""
    lib = E.host._lib.load()
    rng = np.random.default_rng(n + mc)
    S, AS = rng.standard_normal((mc, n)), rng.standard_normal((mc, n))
    ld = n + (n & 1)
    out = {}
    for which in ("plain", "b"):
        a = Arrays(E).put("S", columns(S, n, ld)).put("AS", columns(AS, n, ld)).put("BS", columns(S, n, ld)).put("m", np.ones(ld))
        a.put("G", np.full(mc * mc, SENTINEL)).put("H", np.full(mc * mc, SENTINEL))
        if which == "plain":
            rc = lib.ehyb_lobpcg_gram_step(n, ld, a.ptr("S"), a.ptr("AS"), mc, a.ptr("G"), a.ptr("H"), C.c_void_p(scratch.ptr), None)
        else:
            rc = gram_b(lib, a, n, ld, mc, lumped, scratch)
        assert rc == 0 and lib.ehyb_dev_sync() == 0, lib.ehyb_last_error()
        out[which] = np.concatenate([a.dev["G"].download(), a.dev["H"].download()])
    assert np.isfinite(out["plain"][:mc * mc]).all()
    assert np.array_equal(out["b"].view(np.int64), out["plain"].view(np.int64))


def resid_b(lib, a, n, ld, nb, lumped, with_dinv, mask, ldw, part):
    return lib.ehyb_lobpcg_resid_b_step(n, ld, a.ptr("X"), a.ptr("AX"), a.ptr(None if lumped else "BX"), a.ptr("m" if lumped else None), nb,
                                        a.ptr("theta"), a.ptr("dinv" if with_dinv else None), mask, ldw, a.ptr("W"), a.ptr("res2"),
                                        C.c_void_p(part.ptr), None)


@pytest.mark.parametrize("lumped", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("nb", lc.RESID_COLS)
@pytest.mark.parametrize("n", lg.RESID_SIZES)
def test_resid_b_step(E, gpu, n, nb, lumped):
    """R = AX - BX theta, res2 = the squared norms of all nb columns, W = inv_diag o R (or R) for the listed columns, packed; W held
    NaN everywhere: the column behind the listed ones, the padding row of an odd n and the rows up to ldw keep it"""
    lib = E.host._lib.load()
    ld, ldw = n + (n & 1), n + (n & 1) + 2
    part = E.DeviceBuffer(RESID_SCRATCH)
    for which in lc.ACTIVE:
        for with_dinv in (False, True):
            c = lg.resid_b_case(n, nb, which, with_dinv, lumped, seed=n % 83 + nb)
            na = len(c["W"])
            a = Arrays(E).put("X", columns(c["X"], n, ld)).put("AX", columns(c["AX"], n, ld)).put("theta", c["theta"])
            if lumped:
                a.put("m", np.concatenate([c["m"], np.full(ld - n, SENTINEL)]))
            else:
                a.put("BX", columns(c["BX"], n, ld))
            a.put("W", np.full((na + 1) * ldw, np.nan)).put("res2", np.full(8, SENTINEL))
            if with_dinv:
                a.put("dinv", c["dinv"])
            assert resid_b(lib, a, n, ld, nb, lumped, with_dinv, c["mask"], ldw, part) == 0, lib.ehyb_last_error()
            a.host["res2"][:nb] = c["res2"]
            for k in range(na):
                a.host["W"][k * ldw:k * ldw + n] = c["W"][k]
            assert np.isnan(a.host["W"][na * ldw:(na + 1) * ldw]).all() and np.isnan(a.host["W"][n:ldw]).all()
            a.expect(f"resid_b n={n} nb={nb} active={which} dinv={with_dinv} lumped={lumped}")


@pytest.mark.parametrize("lumped", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n,nb", [(2 * lg.gc.S + 3, 8), (1000, 3), (257, 1)])
def test_resid_b_with_the_identity_is_resid_step_bit_for_bit(E, gpu, n, nb, lumped):
    lib = E.host._lib.load()
    rng = np.random.default_rng(n + nb)
    X, AX, theta, dinv = rng.standard_normal((nb, n)), rng.standard_normal((nb, n)), rng.standard_normal(nb), rng.uniform(0.5, 2.0, n)
    ld = n + (n & 1)
    part = E.DeviceBuffer(RESID_SCRATCH)
    mask = lc.active_mask(nb, "alternate")
    na = bin(mask).count("1")
    out = {}
    for which in ("plain", "b"):
        a = Arrays(E).put("X", columns(X, n, ld)).put("AX", columns(AX, n, ld)).put("BX", columns(X, n, ld)).put("m", np.ones(ld))
        a.put("theta", theta).put("dinv", dinv).put("W", np.full(na * ld, np.nan)).put("res2", np.full(8, SENTINEL))
        if which == "plain":
            rc = lib.ehyb_lobpcg_resid_step(n, ld, a.ptr("X"), a.ptr("AX"), nb, a.ptr("theta"), a.ptr("dinv"), mask, ld, a.ptr("W"),
                                            a.ptr("res2"), C.c_void_p(part.ptr), None)
        else:
            rc = resid_b(lib, a, n, ld, nb, lumped, True, mask, ld, part)
        assert rc == 0 and lib.ehyb_dev_sync() == 0, lib.ehyb_last_error()
        out[which] = np.concatenate([a.dev["W"].download(), a.dev["res2"].download()])
    assert np.isfinite(out["plain"][:n]).all() and (out["plain"][-PAD - 8:-PAD - 8 + nb] > 0).all()
    assert np.array_equal(out["b"].view(np.int64), out["plain"].view(np.int64))


def test_step_calls_check_their_arguments(E, gpu):
    """the checks of ehyb_lobpcg_gram_step and ehyb_lobpcg_resid_step, and exactly one of the two mass forms"""
    lib = E.host._lib.load()
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    S, AS, G, H, SC, TH, DI, W, R2, BS, M = (0x10000 * k for k in range(1, 12))
    gram = lambda n=10, ld=10, s=S, a=AS, bs=BS, m=0, mc=3, g=G, h=H, sc=SC: lib.ehyb_lobpcg_gram_b_step(    # noqa: E731
        n, ld, P(s), P(a), P(bs), P(m), mc, P(g), P(h), P(sc), None)
    for kw in (dict(n=-1), dict(s=0), dict(a=0), dict(g=0), dict(h=0), dict(sc=0), dict(mc=0), dict(mc=25), dict(ld=9), dict(ld=11), dict(ld=8),
               dict(s=S + 8), dict(a=AS + 8), dict(bs=BS + 8), dict(bs=0, m=M + 8), dict(bs=0, m=0), dict(m=M)):
        assert gram(**kw) == ERR_ARG and b"ehyb_lobpcg_gram_b_step" in lib.ehyb_last_error(), kw
    assert gram(bs=0) == ERR_ARG and b"exactly one" in lib.ehyb_last_error()
    assert gram(m=M) == ERR_ARG and b"exactly one" in lib.ehyb_last_error()
    assert gram(mc=99, ld=9) == ERR_ARG and b"mc 99" in lib.ehyb_last_error()
    res = lambda n=10, ld=10, x=S, ax=AS, bx=BS, m=0, nb=3, th=TH, di=DI, mask=5, ldw=12, w=W, r2=R2, sc=SC: lib.ehyb_lobpcg_resid_b_step(    # noqa: E731
        n, ld, P(x), P(ax), P(bx), P(m), nb, P(th), P(di), mask, ldw, P(w), P(r2), P(sc), None)
    for kw in (dict(n=-1), dict(x=0), dict(ax=0), dict(th=0), dict(r2=0), dict(sc=0), dict(nb=0), dict(nb=9), dict(mask=8), dict(w=0),
               dict(ld=9), dict(ld=8), dict(ldw=11), dict(ldw=8), dict(x=S + 8), dict(ax=AS + 8), dict(di=DI + 8), dict(w=W + 8),
               dict(bx=BS + 8), dict(bx=0, m=M + 8), dict(bx=0, m=0), dict(m=M)):
        assert res(**kw) == ERR_ARG and b"ehyb_lobpcg_resid_b_step" in lib.ehyb_last_error(), kw
    assert res(bx=0) == ERR_ARG and b"exactly one" in lib.ehyb_last_error()
