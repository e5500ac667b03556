"""Inputs for the solvers' vector kernels (ehyb_cg.hip, ehyb_bicgstab.hip) whose every output is ONE number in fp64, whatever
the order of summation and whether or not a product is fused -- the counterpart of exact_cases.py for the ten kernels
behind ehyb_pcg, ehyb_pcg_multi and ehyb_bicgstab.  No tests here (test_solver_cases.py, test_gpu_solver_kernels.py).

Why the sizes are what they are.  Every kernel walks i = block*256 + thread with stride = grid*256, first a four-stride
unrolled body (for (; i + 3*stride < n; i += 4*stride)), then a tail (for (; i < n; i += stride)).  walk_profile restates
that walk: the set of (unrolled trips, tail trips) over the threads of a launch.  At n = 12,000 with the solve's own grid
(solver_grid) it is {(0,0), (0,1)}: no thread enters an unrolled body or makes a second tail trip.  SIZES is chosen from
the walk at the grid of the *_step entry points (STEP_GRID = 512): it covers (0,0) (0,1) (0,2) (0,3) (1,0) (1,1) (1,3) (2,0)
(2,1).

How exactness is kept.  Every value is a scaled integer m * 2^-e (Fx: m an int64 array or a Python int, one e per
vector) and the reference is computed on the m in integer arithmetic, never in floating point.  A "scalar" (alpha, beta,
omega, rho ...) is never passed to a kernel: the kernel forms it from the 512 partials of a slot, so a case plants the
partials -- integers of mixed sign and size whose sum is the wanted numerator or denominator (plant) -- and picks them so
that the quotient is a small dyadic number (3/8, -5/4, ...).  inv_diag holds the powers of two 2^-3 .. 2^3, varying with
the index.  Every value a kernel forms, and the sum of the MAGNITUDES of the terms of every partial and of every whole slot
(so every partial sum in every order), is asserted to stay below EXACT_LIMIT = 2^52 units of its last bit: Fx.f() and
partials() assert, they never clip or skip.

What a pass through fp32 would change.  Odd integers of 25 bits or more cannot be held in fp32 ("wide").  Every product a
kernel sums is wide in at least half of its terms, and so is at least half of every vector read -- with one exception that
arithmetic forces: a vector whose SQUARE is summed (b in the init kernels, t in dot2, s in the half step; and q = b - r of
the init kernels with them) cannot be wide in more than 32 elements per partial, because an odd 25-bit number has a square
of 49 bits or more and the positive squares of a partial must add up below 2^53 units.  Those vectors hold odd 13-bit
numbers: their squares are wide (25 or 26 bits), the vectors are not.  Where a dot product of two vectors read is summed
(p.q, rh.v, t.s, rh.r) the two take turns: one is wide at the even indices, the other at the odd ones.
NARROW_BY_NECESSITY lists the exceptions; test_solver_cases.py checks the rule for everything else.
"""
from fractions import Fraction

import numpy as np

from exact_cases import EXACT_LIMIT

THREADS = 256                 # kThreads (vec_reduce.h)
MAX_GRID = 1024               # kMaxGrid: doubles per slot
STEP_GRID = MAX_GRID // 2     # workgroups of every *_step launch, and the solve's cap
S = STEP_GRID * THREADS       # 131,072: one grid stride of a *_step launch
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 77, 3 * S, 3 * S + 1, 4 * S - 1, 4 * S, 4 * S + 1,
         4 * S + 3 * S + 1, 943695, 8 * S + 300]
WANTED_PROFILES = {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3), (2, 0), (2, 1)}
# size -> the profiles of a STEP_GRID launch on it (walk_profile; test_solver_cases.py checks the table, every step test asserts its row)
WALK = {0: {(0, 0)}, 1: {(0, 0), (0, 1)}, 63: {(0, 0), (0, 1)}, 64: {(0, 0), (0, 1)}, 65: {(0, 0), (0, 1)}, 255: {(0, 0), (0, 1)},
        256: {(0, 0), (0, 1)}, 257: {(0, 0), (0, 1)}, S - 1: {(0, 0), (0, 1)}, S: {(0, 1)}, S + 1: {(0, 1), (0, 2)},
        2 * S + 77: {(0, 2), (0, 3)}, 3 * S: {(0, 3)}, 3 * S + 1: {(0, 3), (1, 0)}, 4 * S - 1: {(0, 3), (1, 0)}, 4 * S: {(1, 0)},
        4 * S + 1: {(1, 0), (1, 1)}, 7 * S + 1: {(1, 3), (2, 0)}, 943695: {(1, 3), (2, 0)}, 8 * S + 300: {(2, 0), (2, 1)}}
PAD = 64                      # doubles behind n in every device vector of a case
SENTINEL = -6.02214076e23     # what pads, unnamed slots and outputs hold before a launch

# (kernel, vector): read by the kernel, and not wide anywhere -- see the module docstring
NARROW_BY_NECESSITY = {("cg_init", "b"), ("cg_init", "q"), ("bicg_init", "b"), ("bicg_init", "q"), ("bicg_dot2", "t"),
                       ("bicg_update_half", "sv")}


def solver_grid(n):
    """SolveLoop's rule (solve_loop.h): workgroups of every vector kernel of a solve on n rows."""
    return max(1, min((n + THREADS - 1) // THREADS, MAX_GRID // 2))


def asserted_walk(n):
    """The profiles of a STEP_GRID launch on n elements, asserted against the table: what a step test at size n runs."""
    got = walk_profile(n, STEP_GRID)
    assert got == WALK[n], (n, got, WALK[n])
    return got


def walk_profile(n, grid):
    """The set of (unrolled trips, tail trips) over the threads of a launch of `grid` workgroups on n elements."""
    stride = grid * THREADS
    i = np.arange(stride, dtype=np.int64)
    unrolled = np.zeros(stride, dtype=np.int64)
    tail = np.zeros(stride, dtype=np.int64)
    while True:
        go = i + 3 * stride < n
        if not go.any():
            break
        unrolled += go
        i = np.where(go, i + 4 * stride, i)
    while True:
        go = i < n
        if not go.any():
            break
        tail += go
        i = np.where(go, i + stride, i)
    return set(zip(unrolled.tolist(), tail.tolist()))


# ------------------------------------------------------------------ scaled integers
class Fx:
    """m * 2^-e exactly: m an int64 array (or a Python int), e one non-negative int for the whole vector."""

    def __init__(self, m, e=0):
        self.m = m if isinstance(m, int) else np.asarray(m, dtype=np.int64)
        self.e = int(e)

    def peak(self):
        if isinstance(self.m, int):
            return abs(self.m)
        return int(np.abs(self.m).max()) if self.m.size else 0

    def at(self, e):
        assert e >= self.e and self.peak() << (e - self.e) < 2 ** 62
        return self.m * (1 << (e - self.e))

    def __add__(self, o):
        e = max(self.e, o.e)
        return Fx(self.at(e) + o.at(e), e)

    def __sub__(self, o):
        e = max(self.e, o.e)
        return Fx(self.at(e) - o.at(e), e)

    def __neg__(self):
        return Fx(-self.m, self.e)

    def __mul__(self, o):
        assert self.peak() * o.peak() < 2 ** 62, "int64 would overflow"
        return Fx(self.m * o.m, self.e + o.e)

    def f(self, what=""):
        """float64, asserting that every element is below EXACT_LIMIT units of the vector's last bit"""
        assert self.peak() < EXACT_LIMIT, f"{what}: {self.peak():.3e} units, not exact in fp64"
        if isinstance(self.m, int):
            return float(Fraction(self.m, 1 << self.e))
        return np.ldexp(self.m.astype(np.float64), -self.e)

    def fractions(self):
        return [Fraction(int(v), 1 << self.e) for v in np.atleast_1d(self.m)]


def dyadic(num, den_log2):
    """The scalar num / 2^den_log2."""
    return Fx(int(num), den_log2)


def significant_bits(m):
    """Per element: the width of the odd part of |m| (0 for 0)."""
    m = np.abs(np.asarray(m, dtype=np.int64))
    assert (m < 2 ** 62).all()
    low = m & -m
    out = np.zeros(m.shape, dtype=np.int64)
    nz = m != 0
    odd = m[nz] // low[nz]
    bits = np.zeros(odd.shape, dtype=np.int64)
    while (odd > 0).any():
        bits += odd > 0
        odd = odd >> 1
    out[nz] = bits
    return out


def wide_share(m):
    """Share of the elements that need more than 24 significant bits (1.0 for an empty vector)."""
    m = np.asarray(m)
    return 1.0 if m.size == 0 else float((significant_bits(m) > 24).mean())


def odd_ints(rng, n, bits):
    """Odd integers with magnitude in [2^(bits-1), 2^bits) and random sign."""
    mag = rng.integers(1 << (bits - 2), 1 << (bits - 1), n, dtype=np.int64) * 2 + 1
    return mag * rng.choice(np.array([-1, 1], dtype=np.int64), n)


def taking_turns(rng, n, wide_bits, narrow_bits):
    """Two vectors of odd integers: the first wide at the even indices and narrow at the odd ones, the second the other way round."""
    a, b = odd_ints(rng, n, wide_bits), odd_ints(rng, n, wide_bits)
    a[1::2] = odd_ints(rng, len(a[1::2]), narrow_bits)
    b[0::2] = odd_ints(rng, len(b[0::2]), narrow_bits)
    return a, b


def inv_diag_fx(n):
    """2^k with k in -3 .. 3, varying with the index (and not with period 256 or a grid stride)."""
    i = np.arange(n, dtype=np.int64)
    k = (i * 5 + i // 7 + i // THREADS) % 7 - 3
    return Fx(np.left_shift(np.int64(1), k + 3), 3)


# ------------------------------------------------------------------ partial sums
def partials(terms, grid, what=""):
    """Every single partial of a slot after a kernel summed `terms` (Fx, one term per index): partial b is the sum over
    the i with (i mod stride) // 256 == b.  Asserts that the magnitudes of a whole slot add up below EXACT_LIMIT units.
    -> Fx of `grid` entries"""
    n = len(terms.m)
    stride = grid * THREADS
    trips = max(1, -(-n // stride))
    padded = np.zeros(trips * stride, dtype=np.int64)
    padded[:n] = terms.m
    assert terms.peak() * max(n, 1) < 2 ** 62
    total = int(np.abs(padded).sum())
    assert total < EXACT_LIMIT, f"{what}: the slot's magnitudes add up to 2^{np.log2(max(total, 1)):.1f} units, not exact in fp64"
    return Fx(padded.reshape(trips, grid, THREADS).sum(axis=(0, 2)), terms.e)


def plant(total, grid=STEP_GRID, seed=0):
    """`grid` integer partials of mixed sign and size that add up to the Python int `total`, as an int64 array; the
    magnitudes add up below EXACT_LIMIT, so every order of summation gives `total`."""
    rng = np.random.default_rng(1000 + seed)
    size = rng.integers(1, 41, grid)
    parts = rng.integers(-(1 << 40), 1 << 40, grid, dtype=np.int64) >> (40 - size)
    parts[0] = 0
    parts[0] = int(total) - int(parts.sum())
    assert int(parts.sum()) == int(total) and int(np.abs(parts).sum()) < EXACT_LIMIT
    return parts


def planted_slot(total, e=0, grid=STEP_GRID, seed=0, rest=np.nan):
    """A whole slot (MAX_GRID doubles) whose first `grid` entries are plant(total) * 2^-e and whose other entries hold `rest`
    (NaN: a kernel that adds more than gridDim.x entries cannot give a finite scalar)."""
    out = np.full(MAX_GRID, rest, dtype=np.float64)
    out[:grid] = Fx(plant(total, grid, seed), e).f("planted slot")
    return out


def in_order_sum(slot, grid=STEP_GRID):
    """The first `grid` entries added one after another, as SolveLoop::sum does."""
    t = 0.0
    for v in np.asarray(slot[:grid], dtype=np.float64).tolist():
        t += v
    return t


def rounded_quotient(num, den):
    """The correctly rounded fp64 quotient of two integers (CPython rounds an int / int division correctly)."""
    return float(Fraction(int(num), int(den)))


# ------------------------------------------------------------------ the cases: inputs, planted scalars, exact outputs
# A case is a dict: "in": name -> Fx (vectors the kernel reads), "scalars": name -> (numerator, denominator) Python ints
# planted as partials, "out": name -> Fx (vectors it writes), "sums": name -> Fx of STEP_GRID partials, "products": name ->
# Fx of the terms of that sum (for the width rule).  dinv is None or an Fx.  Everything is deterministic in (n, seed).
ALPHAS = {0: (3, 3), 1: (-5, 2)}      # cur -> alpha as (numerator, log2 denominator): 3/8, -5/4
ODD_C = 12345677                      # numerators and denominators are planted as multiples of an odd constant


def _ex(v, what="an intermediate"):
    """v itself, asserted to be below EXACT_LIMIT units: a value the kernel forms on the way (fused or not)"""
    assert v.peak() < EXACT_LIMIT, f"{what}: {v.peak():.3e} units, not exact in fp64"
    return v


def _z(r, dinv):
    return r if dinv is None else _ex(r * dinv)


def cg_init_case(n, with_dinv, seed=0, grid=STEP_GRID):
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    b, r = Fx(odd_ints(rng, n, 13), 3), Fx(odd_ints(rng, n, 13), 3)
    q = b - r
    z = _z(r, dinv)
    prod = {"rz": r * z, "rr": r * r, "bb": b * b}
    return {"in": {"b": b, "q": q}, "dinv": dinv, "out": {"r": r, "p": z},
            "sums": {k: partials(v, grid, "cg_init " + k) for k, v in prod.items()}, "products": prod}


def dot_case(n, seed=0, grid=STEP_GRID):
    """p . q (cg dot) and rh . v (bicg dot)"""
    rng = np.random.default_rng(seed)
    a, b = taking_turns(rng, n, 26, 5)
    a, b = Fx(a, 2), Fx(b, 1)
    prod = {"pq": a * b}
    return {"in": {"p": a, "q": b}, "dinv": None, "out": {}, "sums": {"pq": partials(prod["pq"], grid, "dot")}, "products": prod}


def cg_update_case(n, cur, with_dinv, seed=0, grid=STEP_GRID):
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    num, lg = ALPHAS[cur]
    alpha = dyadic(num, lg)
    p, q = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26))
    x = Fx(odd_ints(rng, n, 30))
    r_new = Fx(odd_ints(rng, n, 13), 3)
    r_old = r_new + _ex(alpha * q)
    z = _z(r_new, dinv)
    prod = {"rz": r_new * z, "rr": r_new * r_new}
    return {"in": {"p": p, "q": q, "x": x, "r": r_old}, "dinv": dinv, "alpha": alpha,
            "scalars": {"rz": (num * ODD_C, 1), "pq": ((1 << lg) * ODD_C, 1)},
            "out": {"x": x + _ex(alpha * p), "r": r_new},
            "sums": {k: partials(v, grid, "cg_update " + k) for k, v in prod.items()}, "products": prod}


def cg_direction_case(n, cur, with_dinv, seed=0):
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    num, lg = ALPHAS[cur ^ 1]
    beta = dyadic(num, lg)
    r, p = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 27), 1)
    return {"in": {"r": r, "p": p}, "dinv": dinv, "beta": beta,
            "scalars": {"rz_new": (num * ODD_C, 1), "rz": ((1 << lg) * ODD_C, 1)},
            "out": {"p": _z(r, dinv) + _ex(beta * p)}, "sums": {}, "products": {}}


def bicg_init_case(n, with_dinv, seed=0, grid=STEP_GRID):
    c = cg_init_case(n, with_dinv, seed + 50, grid)
    r = c["out"]["r"]
    return {"in": c["in"], "dinv": c["dinv"], "out": {"r": r, "rh": r, "p": c["out"]["p"]},
            "sums": {"rho": c["sums"]["rr"], "rr": c["sums"]["rr"], "bb": c["sums"]["bb"]},
            "products": {"rr": c["products"]["rr"], "bb": c["products"]["bb"]}}


def bicg_s_case(n, cur, with_dinv, seed=0, grid=STEP_GRID):
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    num, lg = ALPHAS[cur]
    alpha = dyadic(num, lg)
    v = Fx(odd_ints(rng, n, 26))
    sv = Fx(odd_ints(rng, n, 13), 3)
    r = sv + _ex(alpha * v)
    prod = {"ss": sv * sv}
    return {"in": {"r": r, "v": v}, "dinv": dinv, "alpha": alpha,
            "scalars": {"rho": (num * ODD_C, 1), "rv": ((1 << lg) * ODD_C, 1)},
            "out": {"sv": sv, "sh": _z(sv, dinv)},
            "sums": {"ss": partials(prod["ss"], grid, "bicg_s ss")}, "products": prod}


def bicg_dot2_case(n, seed=0, grid=STEP_GRID):
    """t.s and t.t: t is squared, so it is never wide; at the even indices t has 13 bits (t.t and t.s wide), at the odd
    ones 3 bits against a wide s (t.s wide)."""
    rng = np.random.default_rng(seed)
    t, sv = odd_ints(rng, n, 13), odd_ints(rng, n, 13)
    t[1::2] = odd_ints(rng, len(t[1::2]), 3)
    sv[1::2] = odd_ints(rng, len(sv[1::2]), 26)
    t, sv = Fx(t, 3), Fx(sv, 2)
    prod = {"ts": t * sv, "tt": t * t}
    return {"in": {"t": t, "sv": sv}, "dinv": None, "out": {}, "sums": {k: partials(v, grid, "bicg_dot2 " + k) for k, v in prod.items()},
            "products": prod}


OMEGAS = {0: (-5, 2), 1: (3, 2)}      # cur -> omega: -5/4, 3/4


def bicg_update_case(n, cur, seed=0, grid=STEP_GRID):
    """The full step.  r_new and rh take turns being wide in the terms of rho_new = rh.r; r.r is wide at the even indices."""
    rng = np.random.default_rng(seed)
    an, al = ALPHAS[cur]
    on, ol = OMEGAS[cur]
    alpha, omega = dyadic(an, al), dyadic(on, ol)
    p, sh, t = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26), 1), Fx(odd_ints(rng, n, 26))
    x = Fx(odd_ints(rng, n, 30))
    r_new, rh = odd_ints(rng, n, 13), odd_ints(rng, n, 13)
    r_new[1::2] = odd_ints(rng, len(r_new[1::2]), 3)
    rh[1::2] = odd_ints(rng, len(rh[1::2]), 26)
    r_new, rh = Fx(r_new, 3), Fx(rh, 1)
    sv = r_new + _ex(omega * t)
    prod = {"rho": rh * r_new, "rr": r_new * r_new}
    return {"in": {"p": p, "sh": sh, "sv": sv, "t": t, "rh": rh, "x": x}, "dinv": None, "alpha": alpha, "omega": omega,
            "scalars": {"rho": (an * ODD_C, 1), "rv": ((1 << al) * ODD_C, 1), "ts": (on * 7654321, 1),
                        "tt": ((1 << ol) * 7654321, 1)},
            "out": {"x": _ex(x + _ex(alpha * p)) + _ex(omega * sh), "r": r_new},
            "sums": {k: partials(v, grid, "bicg_update " + k) for k, v in prod.items()}, "products": prod}


def bicg_half_case(n, cur, seed=0, grid=STEP_GRID):
    """The half step: x += alpha p^, r = s, partials of r.r = s.s (s is squared: 13 bits)."""
    rng = np.random.default_rng(seed)
    an, al = ALPHAS[cur]
    alpha = dyadic(an, al)
    p, x = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 30))
    sv = Fx(odd_ints(rng, n, 13), 3)
    prod = {"rr": sv * sv}
    return {"in": {"p": p, "sv": sv, "x": x}, "dinv": None, "alpha": alpha,
            "scalars": {"rho": (an * ODD_C, 1), "rv": ((1 << al) * ODD_C, 1)},
            "out": {"x": x + _ex(alpha * p), "r": sv},
            "sums": {"rr": partials(prod["rr"], grid, "bicg half rr")}, "products": prod}


# direction: alpha = rho / rv = 3/8, omega = ts / tt = 3/4, rho_new / rho = 5/2 (cur 0) or -3/2 (cur 1), so that
# beta = (rho_new / rho) (alpha / omega) = 5/4 or -3/4 with every one of the three roundings exact
DIRECTION_RATIO = {0: 5, 1: -3}


def bicg_direction_case(n, cur, with_dinv, seed=0):
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    ratio = DIRECTION_RATIO[cur]
    omega, beta = dyadic(3, 2), dyadic(ratio, 2)
    r, v, p = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 27), 1)
    out = _z(r, dinv) + _ex(beta * _ex(p - _ex(omega * _z(v, dinv))))
    return {"in": {"r": r, "v": v, "p": p}, "dinv": dinv, "beta": beta, "omega": omega,
            "scalars": {"rho": (6 * ODD_C, 1), "rho_new": (3 * ratio * ODD_C, 1), "rv": (16 * ODD_C, 1), "ts": (3 * 7654321, 1),
                        "tt": (4 * 7654321, 1)},
            "out": {"p": out}, "sums": {}, "products": {}}


# ------------------------------------------------------------------ division probes
# (R, P): neither a power of two times the other; |R|, |P| < 2^52.  The scalar a kernel forms from them must be the
# correctly rounded quotient.
DIVISION_PROBES = [(1, 3), (-7, 11), (2 ** 51 - 1, 3), (1234567890123457, -987654321987653), (3, 2 ** 51 - 5),
                   (-(2 ** 50 + 1), 2 ** 50 - 1)]


def bicg_beta_rounded(rho_new, rho, rv, ts, tt):
    """beta = (rho_new / rho) * (alpha / omega) with alpha = rho / rv, omega = ts / tt: every division and the product
    rounded to fp64 in the order the kernel's source states, restated with Fraction."""
    def rnd(fr):
        return Fraction(float(fr))

    alpha, omega = rnd(Fraction(rho, rv)), rnd(Fraction(ts, tt))
    return float(rnd(Fraction(rho_new, rho)) * rnd(alpha / omega))
