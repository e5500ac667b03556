"""Matrix values for the tests of cfg.val_f32 (the device holds every value stream in fp32, rounded to nearest-even).

tie_values: odd integers in [2^24, 2^25) with a hashed sign.  fp32 holds 24 bits, so every one of them lies exactly half way
between two fp32 numbers: float(v) = v +- 1, to the even neighbour.  A conversion that truncates, or rounds half away from zero,
gets about half of them wrong; a multiply that used the fp64 values differs from one on float(v) in every entry.
special_values: the same with the ends of the fp32 range planted by a hash of the entry -- 2^-140 (an fp32 subnormal, kept),
2^-150 (rounds to 0), 2^128 and -1e39 (+inf, -inf) and NaN.
small_odd_x: odd integers below 2^10, so that a row of a few hundred such entries keeps sum |a x| < 2^52 (exact_reference asserts it).
"""
import numpy as np

from exact_cases import _hash

SPECIALS = (np.ldexp(1.0, -140), np.ldexp(1.0, -150), np.ldexp(1.0, 128), -1e39, np.nan)


def _keys(I, J, symmetric):
    I = np.asarray(I, dtype=np.int64)
    J = np.asarray(J, dtype=np.int64)
    return (np.minimum(I, J), np.maximum(I, J)) if symmetric else (I, J)


def tie_values(I, J, symmetric, salt=0):
    a, b = _keys(I, J, symmetric)
    h = _hash(a, b, 0x7E5 + salt)
    mag = ((h >> np.uint64(41)) | np.uint64(1 << 24) | np.uint64(1)).astype(np.int64)   # 23 hashed bits: odd, in [2^24, 2^25)
    assert mag.min() >= 1 << 24 and mag.max() < 1 << 25 and (mag & 1).all()
    return (mag * np.where((h >> np.uint64(5)) & np.uint64(1), -1, 1)).astype(np.float64)


def special_values(I, J, symmetric, one_in=40):
    a, b = _keys(I, J, symmetric)
    V = tie_values(I, J, symmetric)
    pick = _hash(a, b, 0x5EC) % np.uint64(one_in * len(SPECIALS))
    for k, s in enumerate(SPECIALS):
        V[pick == np.uint64(k)] = s
    return V


def small_odd_x(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, 1 << 9, n) * 2 + 1) * rng.choice(np.array([-1, 1]), n)).astype(np.float64)


def f32(v):
    """the fp64 values rounded as the upload rounds them, as fp64 again"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def same_bits_f32(got, want_f64):
    """got (float32) against the fp64 stream rounded by numpy: bit for bit as uint32, NaN by isnan"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = np.asarray(want_f64, dtype=np.float64).astype(np.float32)
    nan = np.isnan(want)
    return got.dtype == np.float32 and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ------------------------------------------------------------------ the random configurations of fuzz_cases.py with cfg.val_f32
FUZZ_SEEDS = range(100, 140)      # those of test_gpu_exact.test_exact_random_plan
FALLBACK_MAX = 4                  # seeds whose drawn configuration puts the residual in panel form (seen: 104 and 118)
FEM_INLINE_SYM = dict(window_mode=2, sym_pairs=1, fuse_er=1, lds_doubles=1024)   # FEM of test_gpu_exact.py: an inline residual AND pairs


def fuzz_case_f32(E, O, seed, **more):
    """fuzz_cases.build(seed, exact=True, val_f32=1, **more) -> (matrix (reordered), cfg, kw, x, exact y, fell back).
    cfg.val_f32 refuses a residual in panel form at upload, so a seed whose host-only plan has one is built again with
    er_mode = 1 (CSR segments), which must remove it: `fell back`.  Nothing else of the draw changes."""
    from fuzz_cases import build

    for fell_back in (False, True):
        m, cfg, kw, x, y_ref, _ = build(E, O, seed, exact=True, val_f32=1, **more, **(dict(er_mode=1) if fell_back else {}))
        probe = E.Plan(m, cfg, upload=False)
        panel = probe.stats["er_partials"] > 0
        probe.destroy()
        if not panel:
            return m, cfg, kw, x, y_ref, fell_back
    raise AssertionError(f"seed {seed}: er_mode = 1 left a residual in panel form")


def window_arm(cfg, stats):
    """which ehyb_ell_f32_kernel<THREADS, INLINE_ER, SYM> a plan's window launch is, None without an ELL entry.  SYM is the
    STORAGE (cfg.sym_pairs = 1 with halo windows: layout.cpp), not whether the matrix had a pair to store: a plan of a matrix
    without one (a diagonal matrix, values that pair nowhere) still launches the SYM kernel, as the launch log shows
    (test_gpu_val_f32._assert_launch_log)."""
    sym = int(cfg.sym_pairs) == 1 and int(cfg.window_mode) == 2
    return (int(cfg.threads), stats["er_inline"] > 0, sym) if stats["nnz_ell"] > 0 else None
