"""Inputs for the five vector kernels of ehyb_gmres.hip whose every output is ONE number in fp64, whatever the order of summation
and whether or not a product is fused -- the counterpart of minres_cases.py, built with the machinery of solver_cases.py (Fx
scaled integers, planted partials).  No tests here (test_gmres_cases.py, test_gpu_gmres_kernels.py).

The walk.  start walks elements as the other solvers' kernels do (solver_cases.partials).  dots, update, next and solve_x walk
PAIRS of elements: pair p = (2p, 2p + 1) belongs to workgroup (p mod (grid * 256)) // 256, the last element of an odd n is a pair of
one (pair_partials).  SIZES are the issue's sizes -- 131073 is one element past 512 workgroups of 256 threads -- and 2 S + 3, one
pair and one single element past a whole stride of the pair walk.  COUNTS are the basis counts at the borders of the register
groups of 8 columns, and the maximum.

The scalars.  Dot products and the update use integers and small dyadic c_i (planted as partials).  h_{j+1} = sqrt(w.w) is an exact
root that is not a power of two (3 * 2^k), and w = h_{j+1} v is built backwards from v, so w / h_{j+1} is a true division with an
exact quotient.  The planted rotations 0 .. j-1 are dyadic (the kernel applies whatever (cs, sn) it finds) and all but three of
them are quarter turns, so that the column stays exact through 63 of them; the column's last entry is chosen so that the new
rotation is (h_j, h_{j+1}, gamma) = (4, 3, 5) 2^k: gamma an exact hypotenuse, cs = fl(4/5), sn = fl(3/5) correctly rounded
quotients, and g~_j a power of two so that g_j, g~_{j+1} are exact scalings and rho one rounded product.
The triangular system has small dyadic y and diagonal entries that are not powers of two; g = R y is built backwards."""
from fractions import Fraction

import numpy as np

import solver_cases as sc
from exact_cases import EXACT_LIMIT
from solver_cases import Fx, S, STEP_GRID, THREADS, _ex, inv_diag_fx, odd_ints

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, S + 1, 2 * S + 3]
COUNTS = [1, 2, 8, 9, 31, 65]
DYADICS = [Fraction(3, 8), Fraction(-5, 4), Fraction(1, 2), Fraction(-3, 4), Fraction(1), Fraction(7, 8), Fraction(-1, 4), Fraction(3, 2)]


def exact(fr):
    """the Fraction as a float, asserted exact"""
    f = float(fr)
    assert Fraction(f) == Fraction(fr), f"{fr} is not a double"
    return f


def fx_of(fr):
    fr = Fraction(fr)
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e, f"{fr} is not dyadic"
    return sc.dyadic(fr.numerator, e)


def pair_partials(terms, grid=STEP_GRID, what=""):
    """the `grid` partials of a pair-walking kernel that sums `terms` (Fx, one per element): element i goes to workgroup
    (i mod (512 grid)) // 512.  Every partial's magnitudes add up below EXACT_LIMIT units, so it is one number in every order."""
    n = len(terms.m)
    stride = 2 * grid * THREADS
    trips = max(1, -(-n // stride))
    padded = np.zeros(trips * stride, dtype=np.int64)
    padded[:n] = terms.m
    assert terms.peak() * max(n, 1) < 2 ** 62
    mags = np.abs(padded).reshape(trips, grid, 2 * THREADS).sum(axis=(0, 2))
    assert int(mags.max()) < EXACT_LIMIT, f"{what}: a partial's magnitudes add up to {int(mags.max())} units"
    return Fx(padded.reshape(trips, grid, 2 * THREADS).sum(axis=(0, 2)), terms.e)


def basis(rng, n, count, bits):
    return [Fx(odd_ints(rng, n, bits), i % 3) for i in range(count)]


def coefficients(count):
    return [DYADICS[(3 * i + i // 8) % len(DYADICS)] for i in range(count)]


def start_case(n, seed=0):
    """w = b - w; partials of w.w and b.b (element walk)"""
    c = sc.cg_init_case(n, False, seed + 90)
    return {"in": {"b": c["in"]["b"], "w": c["in"]["q"]}, "out": {"w": c["out"]["r"]}, "sums": {"ww": c["sums"]["rr"], "bb": c["sums"]["bb"]}}


def dots_case(n, count, seed=0):
    """c_i = v_i . w: w wide (26 bits), the columns 12 bits"""
    rng = np.random.default_rng(seed)
    w = Fx(odd_ints(rng, n, 26), 1)
    V = basis(rng, n, count, 12)
    return {"V": V, "w": w, "sums": [pair_partials(v * w, what=f"dots c{i}") for i, v in enumerate(V)]}


def update_case(n, count, last, seed=0):
    """w -= sum c_i v_i, built backwards from the result; the result is squared when `last`, so it then holds 13-bit numbers"""
    rng = np.random.default_rng(seed)
    c = coefficients(count)
    V = basis(rng, n, count, 20)
    w_new = Fx(odd_ints(rng, n, 13), 3) if last else Fx(odd_ints(rng, n, 26), 1)
    w = w_new
    for i in reversed(range(count)):                           # the kernel subtracts in rising i: every value on the way
        w = _ex(w + _ex(fx_of(c[i]) * V[i]), "update on the way")
    return {"V": V, "c": c, "w": w, "w_new": w_new, "ww": pair_partials(w_new * w_new, what="update ww") if last else None}


QUARTER_TURNS = [(0, 1), (-1, 0), (0, -1), (1, 0)]
TURNS = [(Fraction(-3, 4), Fraction(1, 2)), (Fraction(1, 2), Fraction(-1, 2))]


def next_case(n, j, with_dinv, seed=0, k=1):
    """step j >= 0: the Hessenberg column through the planted rotations, the new rotation (4, 3, 5) 2^k, v_{j+1} = w / (3 2^k)"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    rot = [(Fraction(a), Fraction(b)) for a, b in (QUARTER_TURNS[i % 4] for i in range(j))]
    for i, t in zip((0, 1), TURNS):
        if i < j - 1:
            rot[i] = t
    if j > 0:
        rot[j - 1] = (Fraction(1, 2), Fraction(-1, 2))
    scale = Fraction(2) ** k
    h = [DYADICS[(i + seed) % len(DYADICS)] * 4 for i in range(j)] + [Fraction(0)]
    # the chain up to the last rotation, then h_j such that the rotated h_j is 4 * 2^k
    col = list(h)
    for i in range(j):
        cs, sn = rot[i]
        if i == j - 1:
            col[j] = h[j] = (4 * scale + sn * col[i]) / cs
        t = cs * col[i] + sn * col[i + 1]
        col[i + 1] = -sn * col[i] + cs * col[i + 1]
        col[i] = t
    if j == 0:
        col[0] = h[0] = 4 * scale
    assert col[j] == 4 * scale
    hn, gamma = 3 * scale, 5 * scale
    gt = Fraction(2)
    cs_new, sn_new = float(4 * scale) / float(gamma), float(hn) / float(gamma)       # IEEE divisions, as the kernel's
    gnext, gfin = -sn_new * float(gt), cs_new * float(gt)                            # g~_j is a power of two: exact scalings
    v = Fx(odd_ints(rng, n, 26), 2)
    w = _ex(fx_of(hn) * v)
    z = v if dinv is None else _ex(v * dinv)
    return {"j": j, "dinv": dinv, "rot": [(exact(a), exact(b)) for a, b in rot], "h": [exact(x) for x in h], "ww": hn * hn, "gt": exact(gt),
            "w": w, "v": v, "z": z, "R": [exact(x) for x in col[:j]] + [exact(gamma)], "cs": cs_new, "sn": sn_new, "g": gfin,
            "gt_next": gnext, "rho": gnext * gnext}


def first_case(n, with_dinv, seed=0):
    """j = -1: beta = sqrt(r.r) = 3/2, v_0 = w / beta"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    beta = Fraction(3, 2)
    v = Fx(odd_ints(rng, n, 26), 2)
    return {"dinv": dinv, "ww": beta * beta, "beta": exact(beta), "w": _ex(fx_of(beta) * v), "v": v, "z": v if dinv is None else _ex(v * dinv)}


DIAGONAL = [Fraction(3, 2), Fraction(-5, 4), Fraction(2), Fraction(3, 4), Fraction(-1, 2)]


def solve_x_case(n, J, with_dinv, seed=0):
    """R y = g with small dyadic y, g built backwards; x += M^-1 sum y_i v_i"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    y = [DYADICS[(5 * i + seed) % len(DYADICS)] for i in range(J)]
    R = [[(DIAGONAL[(i + seed) % len(DIAGONAL)] if i == c else DYADICS[(i + 2 * c) % len(DYADICS)] * (-1) ** (i + c)) if i <= c else Fraction(0)
          for c in range(J)] for i in range(J)]
    g = [sum(R[i][c] * y[c] for c in range(i, J)) for i in range(J)]
    # what the kernel holds on the way: g_k after the columns J-1 .. i have been taken out
    for i in range(J):
        for first in range(i, J + 1):
            exact(sum(R[i][c] * y[c] for c in range(i, first)))
    V = basis(rng, n, J, 20)
    acc = None
    for i in range(J):
        term = _ex(fx_of(y[i]) * V[i])
        acc = term if acc is None else _ex(acc + term, "solve_x on the way")
    x = Fx(odd_ints(rng, n, 30))
    if acc is None:
        x_new = x
    else:
        x_new = _ex(x + (acc if dinv is None else _ex(acc * dinv)))
    return {"J": J, "dinv": dinv, "V": V, "y": y, "R": [[exact(v) for v in row] for row in R], "g": [exact(v) for v in g], "x": x, "x_new": x_new}
