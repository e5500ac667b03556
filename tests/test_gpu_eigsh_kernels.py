"""The three kernels of ehyb_eigsh.hip one launch at a time through ehyb_eigsh_*_step, bit for bit, on the inputs of eigsh_cases.py:
every output is one number in fp64, so every vector, every basis column, every slot and every double of the tail is compared
exactly (up to the sign of zero).  No tolerance appears in this file.

The guards are those of test_gpu_gmres_kernels.py, whose Bench is used: pads of sentinels behind every vector, behind the basis and
behind the tail; whatever a kernel does not name keeps its sentinel; inputs come back unchanged; for an odd n the padding element
of every column holds the sentinel.  The rotation has two arrays of columns with leading dimensions of their own: rows n .. ld of
every column, the columns >= kc of dst and all of src must keep what they held."""
import ctypes as C

import numpy as np
import pytest

import eigsh_cases as ec
import gmres_cases as gc
import solver_cases as sc
import test_gpu_gmres_kernels as gk
from solver_cases import MAX_GRID, PAD, SENTINEL

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = gk.RUNNING, gk.CONVERGED, gk.BREAKDOWN
ITERS = gk.ITERS


@pytest.fixture(scope="module")
def layout(E):
    from ehyb_spmv_gpu_amd import _lib

    L = _lib.GmresSlots()
    assert _lib.load().ehyb_gmres_layout(C.byref(L)) == 0
    out = L.as_dict()
    assert out["slot_doubles"] == MAX_GRID and out["max_restart"] == 64 and out["r_stride"] == 64
    return out


# ------------------------------------------------------------------ rotate
BIG = [s for s in gc.SIZES if s > 1000]


def rotate_shapes():
    """every shape at the sizes up to 257; past a grid stride the shapes that reach one, two, nine and the partial last register
    group, and the two largest at S + 1"""
    out = []
    for n in gc.SIZES:
        for mc, kc in ec.ROTATE_SHAPES:
            if n < 1000 or (mc, kc) in ((2, 1), (9, 9), (21, 15), (65, 1)) or (n == BIG[0] and mc >= 64):
                out.append((n, mc, kc))
    return out


@pytest.mark.parametrize("n,mc,kc", rotate_shapes())
def test_rotate_step(E, gpu, layout, n, mc, kc):
    c = ec.rotate_case(n, mc, kc, seed=n % 61 + mc + kc)
    b = gk.Bench(E, layout, n)
    lds, ldd = n + (n & 1) + 2, n + (n & 1) + 6                   # ld_dst != ld_src, both beyond n rounded up
    extra = 3                                                    # columns of dst behind kc
    src = np.full(lds * mc + PAD, SENTINEL)
    for l in range(mc):
        src[l * lds:l * lds + n] = c["src"][l]
    dst = np.full(ldd * (kc + extra) + PAD, SENTINEL)
    b.upload("src", src).upload("dst", dst).upload("Y", np.concatenate([c["Y"].T.ravel(), np.full(PAD, SENTINEL)]))
    b.call("ehyb_eigsh_rotate_step", lds, "src", ldd, "dst", "Y", mc, kc)
    for col in range(kc):
        b.host["dst"][col * ldd:col * ldd + n] = c["dst"][col]
    b.expect(f"rotate n={n} mc={mc} kc={kc}")


def test_rotate_does_not_look_at_the_status(E, gpu, layout):
    n, mc, kc = 257, 9, 9
    c = ec.rotate_case(n, mc, kc, seed=5)
    for status in (CONVERGED, BREAKDOWN):
        b = gk.Bench(E, layout, n, status=status)
        ld = n + 1
        src = np.full(ld * mc + PAD, SENTINEL)
        for l in range(mc):
            src[l * ld:l * ld + n] = c["src"][l]
        b.upload("src", src).upload("dst", np.full(ld * kc + PAD, SENTINEL)).upload("Y", c["Y"].T.ravel().copy())
        b.call("ehyb_eigsh_rotate_step", ld, "src", ld, "dst", "Y", mc, kc)
        for col in range(kc):
            b.host["dst"][col * ld:col * ld + n] = c["dst"][col]
        b.expect(f"rotate with status {status}")


# ------------------------------------------------------------------ next
def next_bench(E, L, n, j, with_scale, seed, status=RUNNING, **kw):
    c = ec.next_case(n, j, with_scale, seed=seed, **kw)
    b = gk.Bench(E, L, n, status=status).vec("w", c["w"]).vec("z").basis([], j + 2)
    if with_scale:
        b.vec("scale", c["scale"])
    b.plant(L["slot_ww"], c["ww"], seed=3)
    b.tail("h_at", c["h"], offset=L["h_stride"])
    return c, b


def next_args(b, with_scale, j):
    return (b.ld, "V", "w", "scale" if with_scale else None, "z", "slots", j)


def next_tail(L, c, j, beta=None):
    return {("r_at", j * L["r_stride"]): c["h"], ("gt_at", j + 1): c["beta"] if beta is None else beta}


@pytest.mark.parametrize("j", ec.NEXT_J)
@pytest.mark.parametrize("n", gc.SIZES)
def test_next_step(E, gpu, layout, n, j):
    """column j of T, beta at gt[j + 1], the counter; v_{j+1} = w / beta and z = scale o v_{j+1}; the status stays"""
    L = layout
    for with_scale in (False, True):
        c, b = next_bench(E, L, n, j, with_scale, n % 79 + j)
        b.call("ehyb_eigsh_next_step", *next_args(b, with_scale, j))
        b.expect(f"next n={n} j={j} scale={with_scale}", {"z": c["z"]}, columns={j + 1: c["v"]}, tail=next_tail(L, c, j), flags=(RUNNING, ITERS + 1))


@pytest.mark.parametrize("n", gc.SIZES)
def test_next_step_normalises_the_start_vector(E, gpu, layout, n):
    """j = -1: beta = 3/2 into gt[0], v_0 = w / beta, z = scale o v_0; the counter stays"""
    L = layout
    for with_scale in (False, True):
        c = gc.first_case(n, with_scale, seed=n % 73)
        b = gk.Bench(E, L, n).vec("w", c["w"]).vec("z").basis([], 1)
        if with_scale:
            b.vec("scale", c["dinv"])
        b.plant(L["slot_ww"], c["ww"], seed=4)
        b.call("ehyb_eigsh_next_step", *next_args(b, with_scale, -1))
        b.expect(f"first n={n} scale={with_scale}", {"z": c["z"]}, columns={0: c["v"]}, tail={("gt_at", 0): c["beta"]})


def test_the_invariant_rule_on_both_sides_of_its_threshold(E, gpu, layout):
    """h_0 = 3 * 2^45 and beta = 3: h.h + beta^2 rounds to 9 * 2^90, so beta^2 <= 2^-90 (h.h + beta^2) holds with equality: the step
    counts, column 0 and beta = 0 are written, the status is converged, no vector moves.  The next smaller h_0: h.h rounds to
    9 * 2^90 - 2^41, the rule fails by 2^-49 and the step goes on."""
    L, n, j = layout, 257, 0
    h0 = 3.0 * 2.0 ** 45
    c, b = next_bench(E, L, n, j, True, 5, k=0, h0=h0)
    assert c["beta"] == 3.0 and c["h"] == [h0] and 9.0 <= 2.0 ** -90 * (h0 * h0 + 9.0)
    b.call("ehyb_eigsh_next_step", *next_args(b, True, j))
    b.expect("invariant at equality", tail=next_tail(L, c, j, beta=0.0), flags=(CONVERGED, ITERS + 1))
    below = float(np.nextafter(h0, 0.0))
    assert not 9.0 <= 2.0 ** -90 * (below * below + 9.0)
    c, b = next_bench(E, L, n, j, True, 5, k=0, h0=below)
    b.call("ehyb_eigsh_next_step", *next_args(b, True, j))
    b.expect("one ulp below", {"z": c["z"]}, columns={j + 1: c["v"]}, tail=next_tail(L, c, j), flags=(RUNNING, ITERS + 1))
    # w.w = 0 behind eight columns: invariant whatever h holds
    c, b = next_bench(E, L, n, 8, False, 6)
    b.slot(L["slot_ww"], sc.planted_slot(0, seed=2))
    b.call("ehyb_eigsh_next_step", *next_args(b, False, 8))
    b.expect("w.w = 0", tail=next_tail(L, c, 8, beta=0.0), flags=(CONVERGED, ITERS + 1))


def test_next_breaks_down_on_a_non_finite_quantity(E, gpu, layout):
    """a NaN or an infinity in h, a NaN in w.w: the status, and nothing else -- V, z and T keep their sentinels.  At the start: a
    zero or non-finite norm."""
    L, n, j = layout, 257, 7
    nan_slot = sc.planted_slot(0, seed=1) + np.where(np.arange(MAX_GRID) == 3, np.nan, 0.0)
    for what in ("nan-h", "inf-h", "nan-ww"):
        c, b = next_bench(E, L, n, j, True, 5)
        if what == "nan-ww":
            b.slot(L["slot_ww"], nan_slot)
        else:
            b.tail("h_at", np.nan if what == "nan-h" else np.inf, offset=L["h_stride"] + 2)
        b.call("ehyb_eigsh_next_step", *next_args(b, True, j))
        b.expect(f"breakdown {what}", flags=(BREAKDOWN, ITERS))
    for what, slot in (("zero", sc.planted_slot(0, seed=2)), ("nan", nan_slot)):
        c = gc.first_case(n, False, seed=1)
        b = gk.Bench(E, L, n).vec("w", c["w"]).vec("z").basis([], 1).slot(L["slot_ww"], slot)
        b.call("ehyb_eigsh_next_step", *next_args(b, False, -1))
        b.expect(f"start vector with a {what} norm", flags=(BREAKDOWN, ITERS))


# ------------------------------------------------------------------ scale
@pytest.mark.parametrize("n", gc.SIZES)
def test_scale_step(E, gpu, layout, n):
    c = ec.scale_case(n, seed=n % 67)
    b = gk.Bench(E, layout, n).vec("w", c["w"]).vec("scale", c["scale"])
    b.call("ehyb_eigsh_scale_step", "scale", "w", "slots")
    b.expect(f"scale n={n}", {"w": c["out"]})


# ------------------------------------------------------------------ a set status
@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
def test_next_and_scale_return_at_once_when_the_status_is_set(E, gpu, layout, status):
    """the inputs of the value tests, on which each step would write: with the status set nothing moves"""
    L = layout
    for n in (257, gc.SIZES[-1]):
        c, b = next_bench(E, L, n, 8, True, 6, status=status)
        b.call("ehyb_eigsh_next_step", *next_args(b, True, 8))
        b.expect(f"next with status {status}")
        c = gc.first_case(n, False, seed=2)
        b = gk.Bench(E, L, n, status=status).vec("w", c["w"]).vec("z").basis([], 1).plant(L["slot_ww"], c["ww"], seed=4)
        b.call("ehyb_eigsh_next_step", *next_args(b, False, -1))
        b.expect(f"next(-1) with status {status}")
        c = ec.scale_case(n, seed=3)
        b = gk.Bench(E, L, n, status=status).vec("w", c["w"]).vec("scale", c["scale"])
        b.call("ehyb_eigsh_scale_step", "scale", "w", "slots")
        b.expect(f"scale with status {status}")
