"""The two kernels of ehyb_lobpcg.hip, each with its fixed-order sum, through ehyb_lobpcg_gram_step and ehyb_lobpcg_resid_step, bit
for bit, on the inputs of lobpcg_cases.py: every output is one number in fp64 whatever the order of summation, so every entry is
compared exactly.  No tolerance appears in this file.

Guards: every device array ends in a pad of sentinels and the rows n .. ld of every column hold the sentinel (-6e23: one of them
read into a sum shows); the inputs must come back unchanged, the pads and every column of W that the mask does not list must keep
the sentinel.  The Gram sizes: 1, around one wave of pairs and one tile of 128 rows (63, 64, 65), several tiles
(1000), one row past 32 tiles (4097), and 70001 > 256 workgroups x 128 rows x 2, where a workgroup walks a third tile and the last
tile is a single row.  The column counts sit on both sides of the 8-column register groups."""
import ctypes as C

import numpy as np
import pytest

import gmres_cases as gc
import lobpcg_cases as lc
from solver_cases import PAD, SENTINEL

pytestmark = pytest.mark.gpu

SCRATCH_DOUBLES = 294912          # EHYB_LOBPCG_SCRATCH_DOUBLES
RESID_SCRATCH = 4096
RESID_SIZES = [n for n in gc.SIZES if n not in (0, 255, 256)]


class Arrays:
    """named device arrays with a sentinel pad; host keeps what each should hold after the call"""

    def __init__(self, E):
        self.E, self.dev, self.host = E, {}, {}

    def put(self, name, a):
        a = np.concatenate([np.asarray(a, dtype=np.float64).ravel(), np.full(PAD, SENTINEL)])
        self.dev[name], self.host[name] = self.E.DeviceBuffer(len(a)).upload(a), a.copy()
        return self

    def ptr(self, name):
        return C.c_void_p(self.dev[name].ptr) if name else None

    def expect(self, what):
        lib = self.E.host._lib.load()
        assert lib.ehyb_dev_sync() == 0
        for name, want in self.host.items():
            got = self.dev[name].download()
            bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
            bad = bad[(got[bad] != 0) | (want[bad] != 0)]              # up to the sign of zero
            assert len(bad) == 0, (what, name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def columns(cols, n, ld, extra=0):
    """(k, n) -> k + extra columns of ld doubles, sentinels in the rows n .. ld and in the extra columns"""
    out = np.full((len(cols) + extra, ld), SENTINEL)
    out[:len(cols), :n] = cols
    return out.ravel()


@pytest.fixture(scope="module")
def scratch(E, gpu):
    return E.DeviceBuffer(SCRATCH_DOUBLES)


@pytest.mark.parametrize("mc", lc.GRAM_COLS)
@pytest.mark.parametrize("n", lc.GRAM_SIZES)
def test_gram_step(E, gpu, scratch, n, mc):
    """G = S^T S and H = S^T AS against the int64 products; the lower triangles equal the upper ones; a column more than mc
    behind S and AS, full of sentinels, is not read"""
    lib = E.host._lib.load()
    c = lc.gram_case(n, mc, seed=n % 89 + mc)
    for ld in (n + (n & 1), n + (n & 1) + 6):
        a = Arrays(E).put("S", columns(c["S"], n, ld, extra=1)).put("AS", columns(c["AS"], n, ld, extra=1))
        a.put("G", np.full(mc * mc, SENTINEL)).put("H", np.full(mc * mc, SENTINEL))
        assert lib.ehyb_lobpcg_gram_step(n, ld, a.ptr("S"), a.ptr("AS"), mc, a.ptr("G"), a.ptr("H"), C.c_void_p(scratch.ptr), None) == 0, \
            lib.ehyb_last_error()
        a.host["G"][:mc * mc] = c["G"].T.ravel()                     # column-major
        a.host["H"][:mc * mc] = c["H"].T.ravel()
        a.expect(f"gram n={n} mc={mc} ld={ld}")
        G = a.dev["G"].download()[:mc * mc].reshape(mc, mc)
        H = a.dev["H"].download()[:mc * mc].reshape(mc, mc)
        assert np.array_equal(G, G.T) and np.array_equal(H, H.T)


def test_gram_step_twice_on_one_scratch_gives_the_same_bits(E, gpu, scratch):
    """what an earlier, wider call left in the slots does not reach a later, narrower one"""
    lib = E.host._lib.load()
    n, ld = 4097, 4098
    for mc in (24, 9, 1):
        c = lc.gram_case(n, mc, seed=mc)
        a = Arrays(E).put("S", columns(c["S"], n, ld)).put("AS", columns(c["AS"], n, ld)).put("G", np.full(mc * mc, SENTINEL))
        a.put("H", np.full(mc * mc, SENTINEL))
        assert lib.ehyb_lobpcg_gram_step(n, ld, a.ptr("S"), a.ptr("AS"), mc, a.ptr("G"), a.ptr("H"), C.c_void_p(scratch.ptr), None) == 0
        a.host["G"][:mc * mc], a.host["H"][:mc * mc] = c["G"].T.ravel(), c["H"].T.ravel()
        a.expect(f"gram after a wider one, mc={mc}")


@pytest.mark.parametrize("nb", lc.RESID_COLS)
@pytest.mark.parametrize("n", RESID_SIZES)
def test_resid_step(E, gpu, n, nb):
    """R = AX - X theta, res2 = the squared norms of all nb columns, W = inv_diag o R (or R) for the listed columns, packed; an
    unlisted column of W, X and AX keep what they held"""
    lib = E.host._lib.load()
    ld, ldw = n + (n & 1), n + (n & 1) + 2
    part = E.DeviceBuffer(RESID_SCRATCH)
    for which in lc.ACTIVE:
        for with_dinv in (False, True):
            c = lc.resid_case(n, nb, which, with_dinv, seed=n % 83 + nb)
            na = len(c["W"])
            a = Arrays(E).put("X", columns(c["X"], n, ld)).put("AX", columns(c["AX"], n, ld)).put("theta", c["theta"])
            a.put("W", np.full((na + 1) * ldw, SENTINEL)).put("res2", np.full(8, SENTINEL))
            if with_dinv:
                a.put("dinv", c["dinv"])
            rc = lib.ehyb_lobpcg_resid_step(n, ld, a.ptr("X"), a.ptr("AX"), nb, a.ptr("theta"), a.ptr("dinv" if with_dinv else None), c["mask"],
                                            ldw, a.ptr("W"), a.ptr("res2"), C.c_void_p(part.ptr), None)
            assert rc == 0, lib.ehyb_last_error()
            a.host["res2"][:nb] = c["res2"]
            for k in range(na):
                a.host["W"][k * ldw:k * ldw + n] = c["W"][k]
            a.expect(f"resid n={n} nb={nb} active={which} dinv={with_dinv}")


def test_resid_step_without_active_columns_takes_no_w(E, gpu):
    lib = E.host._lib.load()
    n, nb = 257, 3
    c = lc.resid_case(n, nb, "none", False, seed=4)
    a = Arrays(E).put("X", columns(c["X"], n, n + 1)).put("AX", columns(c["AX"], n, n + 1)).put("theta", c["theta"]).put("res2", np.full(8, SENTINEL))
    part = E.DeviceBuffer(RESID_SCRATCH)
    assert lib.ehyb_lobpcg_resid_step(n, n + 1, a.ptr("X"), a.ptr("AX"), nb, a.ptr("theta"), None, 0, 0, None, a.ptr("res2"),
                                      C.c_void_p(part.ptr), None) == 0, lib.ehyb_last_error()
    a.host["res2"][:nb] = c["res2"]
    a.expect("resid without W")
