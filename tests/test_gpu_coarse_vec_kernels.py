"""The two weighted kernels of a vector coarse object one launch at a time, bit for bit (ehyb_coarse_restrict_step and
ehyb_coarse_prolong_step on objects of ehyb_coarse_create_raw_vecs; K = 1), on the exact cases of coarse_vec_cases.py: aggregates
of 1, 2, 63, 64, 65, 127, 128, 129, 257 and about 1,000 rows (at the large sizes the last kind takes what is left over)
scattered over the index range, nv = 1, 3, 6 and 8 -- one instantiated bound each and, with 3 of 3, 6 of 6, the bounds met
exactly -- with an irregular OFF: aggregates that keep every column, fewer, none, and a last one that keeps fewer than nv.  W
holds small dyadics and zeros in the dropped columns.  At the sizes of cheb_cases.SIZES, which cover every profile of the
prolong kernel's index walk.  Guards as in test_gpu_coarse_kernels.py: outputs are NaN before the launch, PAD doubles of SENTINEL
behind every vector stay, every slot entry that is not written stays, inputs come back unchanged.  C is followed directly by a
NaN, and in a launch of its own the C entries of the aggregates behind one that dropped columns are NaN: neither may reach a z
outside those aggregates.  No tolerance appears in this file."""
import numpy as np
import pytest

import cheb_cases as cc
import coarse_cases as kc
import coarse_vec_cases as vc
from solver_cases import MAX_GRID, SENTINEL, STEP_GRID
from test_gpu_coarse_kernels import Vec, launch
from test_gpu_solver_kernels import cg_layout  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = [(n, nv) for n in cc.SIZES[1:] for nv in vc.KERNEL_NV]


def layout(E, n, nv):
    """(the uploaded object, agg, off, W as Fx) of one case"""
    agg, nagg = vc.scattered_aggregates(n, seed=n % 97)
    off = vc.irregular_off(nagg, nv)
    W = vc.weights_fx(agg, off, nv, seed=n % 89 + nv)
    nc = int(off[-1])
    kept = np.diff(off)
    if nagg == vc.KERNEL_NAGG:
        sizes = np.bincount(agg)
        assert set(vc.AGG_ROWS[:-1]) <= set(sizes.tolist()) and sizes.max() >= 1000
        assert (kept == nv).any() and (kept == 0).any() and kept[-1] < nv and (nv == 1 or ((kept > 0) & (kept < nv)).any())
        big = int(np.argmax(sizes))
        assert (np.diff(np.flatnonzero(agg == big)) > 1).any(), "the rows of an aggregate are not contiguous"
    co = E.Coarse.raw_vectors(n, agg, off, W.f("W"), kc.einv_fx(nc).f())
    assert np.array_equal(co.array("off"), off) and np.array_equal(co.array("W"), W.f()) and np.array_equal(co.array("map"), agg)
    assert np.array_equal(co.array("row_ptr"), kc.transpose(agg, nagg)[0]) and np.array_equal(co.array("rows"), kc.transpose(agg, nagg)[1])
    return co, agg, off, W


@pytest.mark.parametrize("n,nv", CASES)
def test_restrict_step(E, gpu, n, nv):
    co, agg, off, W = layout(E, n, nv)
    nc = int(off[-1])
    c = vc.restrict_vec_case(agg, off, W, seed=n % 89)
    r, t = Vec(E, n, c["in"]["r"].f("r")), Vec(E, nc)
    launch(E, "ehyb_coarse_restrict_step", co.h, r.ptr, t.ptr)
    t.expect(f"restrict n={n} nv={nv}: T", c["out"]["t"].f("t"))
    r.expect(f"restrict n={n} nv={nv}: r")
    co.destroy()


@pytest.mark.parametrize("n,nv", CASES)
def test_prolong_step(E, gpu, cg_layout, n, nv):  # noqa: F811
    cc.asserted_walk(n)
    L = cg_layout
    co, agg, off, W = layout(E, n, nv)
    nc, kept = int(off[-1]), np.diff(off)
    for with_dinv in (False, True):
        cases = {summed: vc.prolong_vec_case(agg, off, W, with_dinv, summed, seed=n % 89 + nv) for summed in (False, True)}
        dinv = Vec(E, n, cases[False]["dinv"].f("dinv")) if with_dinv else None
        for rz in (-1, 0, 1):
            c = cases[rz >= 0]
            what = f"prolong n={n} nv={nv} inv_diag={with_dinv} rz={rz}"
            # C: its nc entries and a NaN directly behind them (then the sentinel pad)
            r, cv, z = Vec(E, n, c["in"]["r"].f("r")), Vec(E, nc + 1, np.append(c["in"]["c"].f("c"), np.nan)), Vec(E, n)
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
        # the odd aggregates behind an aggregate that dropped columns hold NaN in C: their own rows become NaN, no other row does
        c = cases[False]
        poisoned = np.array([a % 2 == 1 and kept[a - 1] < nv for a in range(len(kept))])
        if poisoned.any():
            cn = np.append(c["in"]["c"].f("c"), np.nan)
            cn[:nc][np.repeat(poisoned, kept)] = np.nan
            want = np.where(poisoned[agg] & (kept[agg] > 0), np.nan, c["out"]["z"].f("z"))
            assert np.isnan(want).any() or not (poisoned & (kept > 0)).any()
            r, cv, z = Vec(E, n, c["in"]["r"].f("r")), Vec(E, nc + 1, cn), Vec(E, n)
            launch(E, "ehyb_coarse_prolong_step", co.h, r.ptr, dinv.ptr if with_dinv else None, cv.ptr, z.ptr, None, -1)
            z.expect(f"prolong n={n} nv={nv} inv_diag={with_dinv}: z beside NaN in C", want)
            cv.expect("C")
    co.destroy()
