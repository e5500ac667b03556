"""The two kernels of ehyb_lobpcg.hip, each with its fixed-order sum, through ehyb_lobpcg_gram_step and ehyb_lobpcg_resid_step, bit
for bit, on the inputs of lobpcg_cases.py: every output is one number in fp64 whatever the order of summation, so every entry is
compared exactly.  No tolerance appears in this file.

Guards: every device array ends in a pad of sentinels and the rows n .. ld of every column hold the sentinel (-6e23: one of them
read into a sum shows); the inputs must come back unchanged, the pads and every column of W that the mask does not list must keep
the sentinel.  The Gram sizes: 1, around one wave of pairs and one tile of 128 rows (63, 64, 65), several tiles
(1000), one row past 32 tiles (4097), and 70001 > 256 workgroups x 128 rows x 2, where a workgroup walks a third tile and the last
tile is a single row.  The column counts sit on both sides of the 8-column register groups.

The exact inputs cannot tell one order of summation from another, so test_the_bits_of_the_recorded_build holds all three mass forms of
both kernels (ehyb_lobpcg_gram_b_step and ehyb_lobpcg_resid_b_step included) to golden/lobpcg_bits.npz, recorded on the device by
golden/make_lobpcg_bits.py, on inputs whose every sum rounds."""
import ctypes as C
import os

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


# ------------------------------------------------------------------ the bits of the build that golden/lobpcg_bits.npz was recorded with
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lobpcg_bits.npz")
BITS_FORMS = ["none", "stored", "lumped"]
BITS_GRAM = [("none", 1, 1), ("none", 129, 17), ("none", 4097, 9), ("none", 70001, 24)] + \
    [(form, n, mc) for form in BITS_FORMS[1:] for n, mc in ((129, 17), (70001, 24))]
BITS_RESID = [(form, n, nb) for form in BITS_FORMS for n, nb in ((257, 1), (1000, 3), (2 * gc.S + 3, 8))]
BITS_EDGE = 64                    # entries kept of either end of a column of W


def bits_inputs(n, k):
    """exact functions of the indices, one IEEE division each, so that every product and every sum rounds: S (X) = the start block
    over 3, AS (AX) = its columns 24 + c over 7, BS (BX) = its columns 48 + c over 5, m = 1 + (i mod 7) / 11, inv_diag = 1 + (i mod 5) / 13,
    theta_c = (2 c - 7) / 9"""
    sb, i = lc.start_block(n, 48 + k), np.arange(n)
    return {"S": sb[:k] / 3.0, "AS": sb[24:24 + k] / 7.0, "BS": sb[48:] / 5.0, "m": 1.0 + (i % 7) / 11.0, "dinv": 1.0 + (i % 5) / 13.0,
            "theta": (2.0 * np.arange(k) - 7.0) / 9.0}


def mass_ptrs(a, form, stored):
    return a.ptr(stored if form == "stored" else None), a.ptr("m" if form == "lumped" else None)


def gram_bits(E, scratch, form, n, mc):
    """one launch -> {"G", "H"}: the int64 patterns of the mc x mc outputs"""
    lib = E.host._lib.load()
    c, ld = bits_inputs(n, mc), n + (n & 1)
    a = Arrays(E).put("S", columns(c["S"], n, ld)).put("AS", columns(c["AS"], n, ld)).put("BS", columns(c["BS"], n, ld))
    a.put("m", np.concatenate([c["m"], np.full(ld - n, SENTINEL)])).put("G", np.full(mc * mc, SENTINEL)).put("H", np.full(mc * mc, SENTINEL))
    if form == "none":
        rc = lib.ehyb_lobpcg_gram_step(n, ld, a.ptr("S"), a.ptr("AS"), mc, a.ptr("G"), a.ptr("H"), C.c_void_p(scratch.ptr), None)
    else:
        rc = lib.ehyb_lobpcg_gram_b_step(n, ld, a.ptr("S"), a.ptr("AS"), *mass_ptrs(a, form, "BS"), mc, a.ptr("G"), a.ptr("H"),
                                         C.c_void_p(scratch.ptr), None)
    assert rc == 0 and lib.ehyb_dev_sync() == 0, lib.ehyb_last_error()
    return {k: a.dev[k].download()[:mc * mc].view(np.int64).copy() for k in ("G", "H")}


def resid_bits(E, form, n, nb):
    """one launch with inv_diag and every other column active -> {"res2", "W"}: the int64 patterns of res2 and of the first and the
    last BITS_EDGE entries of every packed column of W"""
    lib = E.host._lib.load()
    c, ld = bits_inputs(n, nb), n + (n & 1)
    mask = lc.active_mask(nb, "alternate")
    na = bin(mask).count("1")
    a = Arrays(E).put("X", columns(c["S"], n, ld)).put("AX", columns(c["AS"], n, ld)).put("BX", columns(c["BS"], n, ld))
    a.put("m", np.concatenate([c["m"], np.full(ld - n, SENTINEL)])).put("theta", c["theta"]).put("dinv", c["dinv"])
    a.put("W", np.full(na * ld, np.nan)).put("res2", np.full(8, SENTINEL))
    part = E.DeviceBuffer(RESID_SCRATCH)
    if form == "none":
        rc = lib.ehyb_lobpcg_resid_step(n, ld, a.ptr("X"), a.ptr("AX"), nb, a.ptr("theta"), a.ptr("dinv"), mask, ld, a.ptr("W"), a.ptr("res2"),
                                        C.c_void_p(part.ptr), None)
    else:
        rc = lib.ehyb_lobpcg_resid_b_step(n, ld, a.ptr("X"), a.ptr("AX"), *mass_ptrs(a, form, "BX"), nb, a.ptr("theta"), a.ptr("dinv"), mask, ld,
                                          a.ptr("W"), a.ptr("res2"), C.c_void_p(part.ptr), None)
    assert rc == 0 and lib.ehyb_dev_sync() == 0, lib.ehyb_last_error()
    W = a.dev["W"].download()[:na * ld].reshape(na, ld)[:, :n]
    return {"res2": a.dev["res2"].download()[:nb].view(np.int64).copy(),
            "W": np.concatenate([W[:, :BITS_EDGE], W[:, -BITS_EDGE:]], axis=1).view(np.int64).copy()}


def bits_cases(E, scratch):
    """-> (key in the file, its int64 array) for every recorded case, one launch per case"""
    for form, n, mc in BITS_GRAM:
        for k, v in gram_bits(E, scratch, form, n, mc).items():
            yield f"gram_{form}_{n}_{mc}_{k}", v
    for form, n, nb in BITS_RESID:
        for k, v in resid_bits(E, form, n, nb).items():
            yield f"resid_{form}_{n}_{nb}_{k}", v


def test_the_bits_of_the_recorded_build(E, gpu, scratch):
    """G, H, res2 and both ends of every column of W, in all three mass forms, are bit for bit what the build that recorded
    golden/lobpcg_bits.npz gave: the order of every sum -- rows per lane, tiles, shuffle tree, slots -- and every rounding stay"""
    want = np.load(BITS_FILE)
    seen = set()
    for key, got in bits_cases(E, scratch):
        assert got.dtype == np.int64 and np.array_equal(got, want[key]), (key, int((got != want[key]).sum()), got.size)
        seen.add(key)
    assert seen == set(want.files)
