"""The three kernels of the two-level preconditioner one launch at a time, bit for bit (ehyb_coarse_restrict_step,
ehyb_coarse_solve_step, ehyb_coarse_prolong_step; K = 1), on the exact cases of coarse_cases.py: maps whose unknowns hold 1, 2,
63, 64, 65, 127, 128, 129 and about 1,000 rows (or, at the large sizes, a seventh of all rows) scattered over the index range,
nc = 1, 3, 64, 65, 130 (and the largest, 2047 and 2048, for the solve), E^-1 handed in through ehyb_coarse_create_raw, at the
sizes of cheb_cases.SIZES that cover every profile of the prolong kernel's index walk.  Guards as in
test_gpu_solver_kernels.py: outputs are NaN before the launch, PAD doubles of SENTINEL behind every vector stay, every slot
entry that is not written stays, inputs come back unchanged.  No tolerance appears in this file."""
import ctypes as C

import numpy as np
import pytest

import cheb_cases as cc
import coarse_cases as kc
from solver_cases import MAX_GRID, PAD, SENTINEL, STEP_GRID
from test_gpu_solver_kernels import assert_same, cg_layout  # noqa: F401  (cg_layout: a fixture)

pytestmark = pytest.mark.gpu

ERR_ARG = 1


class Vec:
    """a device vector of n doubles with a sentinel pad; values None: an output, NaN before the launch"""

    def __init__(self, E, n, values=None):
        self.n = n
        self.h = np.full(n + PAD, SENTINEL)
        self.h[:n] = np.nan if values is None else values
        self.d = E.DeviceBuffer(len(self.h)).upload(self.h)
        self.ptr = C.c_void_p(self.d.ptr)

    def expect(self, what, values=None):
        """the first n entries (None: as uploaded) and the pad, bit for bit up to the sign of zero"""
        got = self.d.download()
        assert_same(got[:self.n], self.h[:self.n] if values is None else values, what)
        assert np.array_equal(got[self.n:].view(np.int64), self.h[self.n:].view(np.int64)), f"{what}: the pad"


def launch(E, fn, *args):
    lib = E.host._lib.load()
    rc = getattr(lib, fn)(*args, None)
    assert rc == 0, (fn, rc, lib.ehyb_last_error())
    assert lib.ehyb_dev_sync() == 0, (fn, lib.ehyb_last_error())


def test_no_object_without_rows(E, gpu):
    """n = 0 of cheb_cases.SIZES: every unknown must hold a row, so there is nothing to launch"""
    assert cc.SIZES[0] == 0 and kc.scattered_map(0, 1) is None
    h = C.c_void_p()
    empty = np.zeros(1, dtype=np.int32)
    rc = E.host._lib.load().ehyb_coarse_create_raw(0, empty.ctypes.data_as(C.POINTER(C.c_int32)), 1, np.ones(1).ctypes.data_as(C.POINTER(C.c_double)),
                                                   C.byref(h))
    assert rc == ERR_ARG and not h.value


@pytest.mark.parametrize("n", cc.SIZES[1:])
def test_restrict_step(E, gpu, n):
    ran = 0
    for nc in kc.KERNEL_NC:
        cmap = kc.scattered_map(n, nc, seed=n % 97)
        if cmap is None:
            continue
        co = E.Coarse.raw(n, cmap, kc.einv_fx(nc).f())
        row_ptr, rows = co.array("row_ptr"), co.array("rows")
        assert np.array_equal(row_ptr, kc.transpose(cmap, nc)[0]) and np.array_equal(rows, kc.transpose(cmap, nc)[1])
        largest = int(np.argmax(np.diff(row_ptr)))
        assert nc < 3 or n < 1000 or (np.diff(rows[row_ptr[largest]:row_ptr[largest + 1]]) > 1).any(), "the rows of an unknown are not contiguous"
        c = kc.restrict_case(n, cmap, nc, seed=n % 89)
        r, t = Vec(E, n, c["in"]["r"].f("r")), Vec(E, nc)
        launch(E, "ehyb_coarse_restrict_step", co.h, r.ptr, t.ptr)
        t.expect(f"restrict n={n} nc={nc}: T", c["out"]["t"].f("t"))
        r.expect(f"restrict n={n} nc={nc}: r")
        co.destroy()
        ran += 1
    assert ran >= 1 and (n < 130 or ran == len(kc.KERNEL_NC))


@pytest.mark.parametrize("nc", kc.KERNEL_NC + [2, 2047, 2048])
def test_solve_step(E, gpu, nc):
    c = kc.solve_case(nc, seed=nc)
    einv = c["einv"].f("einv")
    assert np.array_equal(einv, einv.T) and (einv != 0).all() and (np.abs(einv * 4) <= 7).all()
    co = E.Coarse.raw(nc + 5, kc.scattered_map(nc + 5, nc, seed=nc), einv)
    assert np.array_equal(co.array("Einv"), einv) and co.array("E").size == 0
    t, cv = Vec(E, nc, c["in"]["t"].f("t")), Vec(E, nc)
    launch(E, "ehyb_coarse_solve_step", co.h, t.ptr, cv.ptr)
    cv.expect(f"solve nc={nc}: C", c["out"]["c"].f("c"))
    t.expect(f"solve nc={nc}: T")
    co.destroy()


@pytest.mark.parametrize("n", cc.SIZES[1:])
def test_prolong_step(E, gpu, cg_layout, n):  # noqa: F811
    cc.asserted_walk(n)
    L = cg_layout
    for nc in kc.KERNEL_NC:
        cmap = kc.scattered_map(n, nc, seed=n % 97)
        if cmap is None:
            continue
        co = E.Coarse.raw(n, cmap, kc.einv_fx(nc).f())
        for with_dinv in (False, True):
            cases = {summed: kc.prolong_case(n, cmap, nc, with_dinv, summed, seed=n % 89 + nc) for summed in (False, True)}
            for rz in (-1, 0, 1):
                c = cases[rz >= 0]
                what = f"prolong n={n} nc={nc} inv_diag={with_dinv} rz={rz}"
                r, cv, z = Vec(E, n, c["in"]["r"].f("r")), Vec(E, nc, c["in"]["c"].f("c")), Vec(E, n)
                dinv = Vec(E, n, c["dinv"].f("dinv")) if with_dinv else None
                s = Vec(E, L["slots"] * MAX_GRID, np.full(L["slots"] * MAX_GRID, SENTINEL))
                launch(E, "ehyb_coarse_prolong_step", co.h, r.ptr, dinv.ptr if with_dinv else None, cv.ptr, z.ptr, s.ptr, rz)
                z.expect(what + ": z", c["out"]["z"].f("z"))
                want = s.h[:s.n].copy()
                if rz >= 0:      # the first STEP_GRID entries of the one slot; the others and the entries from slot_doubles / 2 on stay
                    at = (L["rz0"] + 2 * rz) * MAX_GRID
                    want[at:at + STEP_GRID] = c["sums"]["rz"].f("rz")
                s.expect(what + ": the slots", want)
                for v, name in ((r, "r"), (cv, "c")) + (((dinv, "dinv"),) if with_dinv else ()):
                    v.expect(f"{what}: {name}")
        co.destroy()
