"""ehyb_plan_check (csrc/plan_io.cpp): the content check ehyb_plan_load applies to a cache file, on the CPU.

1. It accepts every plan the builder makes -- the layout fuzz, the value-map cases, the kernel census, the exact and range
   families, column segments and a row split: a check that is too strict would silently turn every cache file into a miss.
2. Damaged files (plan_damage.py): every targeted mutation is refused with code 6; every seeded random mutant is refused, or
   loads and passes the independent strict walk of its bytes -- "accepted" implies "addresses nothing out of bounds".
3. The load path as a stand-alone program under AddressSanitizer and UBSan (csrc/plan_load_check.cpp) walks the same mutants
   and the file cut at every array boundary: no report, and it refuses exactly what the library refused here.

No damaged file is ever uploaded: everything here loads with upload=False and needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

import plan_damage as D
from fuzz_cases import build
from range_cases import FAMILIES
from util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_SEEDS = list(range(48)) + list(range(200, 224)) + list(range(500, 560))     # test_fuzz_layout.py (walks, round trips), test_value_map.py
EXACT_SEEDS = list(range(48)) + list(range(200, 212))                            # test_exact_layout.py


# ---------------------------------------------------------------------------------------------- 1. built plans pass
@pytest.mark.parametrize("exact", [False, True], ids=["float", "exact"])
def test_check_accepts_the_layout_fuzz(E, O, exact):
    shapes = np.zeros(4, dtype=np.int64)
    for seed in (EXACT_SEEDS if exact else FUZZ_SEEDS):
        m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=exact)
        plan = E.Plan(m, cfg, upload=False)
        plan.check()                       # raises EhybError with the seed's rule in the message
        st = plan.stats
        shapes += [st["sym_pairs"] > 0, st["er_partials"] > 0, st["er_inline"] > 0, st["lds_bytes"] == 0]
        plan.destroy()
    assert (shapes[:3] >= 1).all(), shapes         # the seeds reach symmetric pairs, the panel form and an inline residual


def test_check_accepts_a_plan_without_any_window(E, O, tmp_path):
    """Fuzz seed 531: every entry in the panel residual, no partition keeps a window, lds_doubles = 0.  The builder makes such
    plans; the loader used to refuse them (lds_doubles > 0), so their cache file was a miss every time."""
    m, cfg, kw, x, y_ref, scale = build(E, O, 531)
    plan = E.Plan(m, cfg, upload=False)
    assert plan.stats["lds_bytes"] == 0 and plan.stats["er_partials"] > 0
    plan.check()
    plan.save(tmp_path / "p.ehyb", m.reorder_list, key=5)
    back, perm = E.Plan.load(tmp_path / "p.ehyb", key=5, upload=False)
    assert back.stats == plan.stats and np.array_equal(perm, m.reorder_list)
    y, written = O.walk_plan(back, E.vector_reorder(x, perm))
    assert (written == 1).all() and O.check_strict(E.vector_recover(y, perm), y_ref, scale)[0] == 0


def test_check_accepts_the_value_map_cases(E, O):
    from test_value_map import CASES

    for name, kind, args, kw in CASES:
        cfg = E.make_config(value_map=1, **kw)
        c = Case(E, O, kind, args, cfg)
        E.Plan(c.m, cfg, upload=False).check()


def test_check_accepts_the_kernel_census(E):
    from kernel_census_cases import CASES, build_matrix, matrix_key

    seen = set()
    for case in CASES:
        key = matrix_key(case)             # (cases that differ in device-only fields share their host arrays)
        if key in seen:
            continue
        seen.add(key)
        E.Plan(build_matrix(E, case), case.cfg(E), upload=False).check()
    assert len(seen) >= 20


@pytest.mark.parametrize("fam", FAMILIES)
def test_check_accepts_the_range_families(E, O, fam):
    from test_range_layout import SEEDS, family_plan

    for seed in SEEDS:
        family_plan(E, O, seed, fam)[0].check()


def test_check_accepts_column_segments_and_a_row_split(E, O):
    # column segments as test_gpu_parts.py cuts them, at the size of test_er_panel.py
    for kind, args, kw in (("rmat", (15, 1 << 18, 4), dict(er_mode=2, fuse_er=2, er_panel_cols=1024, direct=2, partitioner=E.EHYB_PART_DEGREE)),
                           ("rmat", (15, 1 << 18, 2), dict(er_mode=2, fuse_er=2, er_panel_cols=2048, ell_prune=2, lds_doubles=4096, direct=2)),
                           ("rmat", (14, 1 << 17, 3), dict(er_mode=1, fuse_er=2, direct=2))):
        cfg = E.make_config(**kw)
        c = Case(E, O, kind, args, cfg)
        n = c.n
        segs = np.array([0, (n // 3) & ~1, (n // 3) & ~1, (2 * n // 3) & ~1, n], dtype=np.int32)
        plan = E.Plan(c.m, cfg, upload=False, col_segs=segs)
        assert plan.col_segs == 4
        plan.check()
    # plans over row blocks (the multi-GPU sharding, test_layout.py): rows that do not start at 0, columns over the whole matrix
    for kw in (dict(window_mode=2, lds_doubles=512, n_top=2), dict(lds_doubles=1024, sym_pairs=1), dict(lds_doubles=512, er_mode=2, fuse_er=2, direct=2)):
        cfg = E.make_config(**kw)
        c = Case(E, O, "fem3d", (12000, 3, 16, 16, 13500, 1, 3), cfg)
        pb = c.m.part_boundary
        cut = int(pb[len(pb) // 2])
        for r0, r1 in ((0, cut), (cut, c.n)):
            plan = E.Plan(c.m, cfg, rows=(r0, r1), upload=False)
            assert plan.rows == (r0, r1)
            plan.check()
    # own + foreign rows with the row blocks of pass 2 split at the boundary, as test_reorder.py builds them
    import ctypes as C

    lib = E.host._lib.load()
    cfg = E.make_config(lds_doubles=1024, n_top=2)
    m = E.Matrix.generate("stencil2d", 40, 40, 5, 200, 3, cfg=cfg)
    m.reorder(cfg)
    n0 = m.n
    m.append_ghosts(700, np.array([0, 1, 5], dtype=np.int32), np.array([3, 0, 699], dtype=np.int32), np.array([1.0, 2.0, 3.0]))
    ri = np.repeat(np.arange(600, dtype=np.int32), 2)
    cj = ((np.arange(1200, dtype=np.int32) * 7) % n0).astype(np.int32)
    v = np.ones(1200)
    assert lib.ehyb_matrix_append_rows(C.byref(m.c), n0, 600, 1200, ri.ctypes.data_as(C.POINTER(C.c_int)), cj.ctypes.data_as(C.POINTER(C.c_int)),
                                       v.ctypes.data_as(C.POINTER(C.c_double)), 256) == 0
    plan = E.Plan(m, E.make_config(lds_doubles=1024, n_top=2, er_mode=2, prune_pct=1, fuse_er=2, direct=2, row_split=n0, er_panel_cols=256, er_block_rows=100),
                  rows=(0, n0 + 600), upload=False)
    assert plan.stats["er_partials"] > 0 and plan.rows == (0, n0 + 600)
    plan.check()


# ---------------------------------------------------------------------------------------------- 2. damaged files
RANDOM_SEED, RANDOM_COUNT = 20261020, 300
_forms = {}


def form(E, O, name, tmp_path_factory):
    """(Case, plan, PlanFile) of a form, built and saved once per session"""
    if name not in _forms:
        _forms[name] = D.saved_form(E, O, name, tmp_path_factory.mktemp(name) / "plan.ehyb")
    return _forms[name]


def mutants(f, name):
    return D.targeted(f), D.random_mutants(f, RANDOM_SEED + sorted(D.FORMS).index(name), RANDOM_COUNT)


def load(E, path):
    """-> (refused?, the loader's message): loaded on the host only"""
    try:
        plan, _ = E.Plan.load(path, upload=False)
    except E.EhybError as e:
        assert e.code == 6, str(e)
        return True, str(e)
    plan.check()            # what the loader applied, callable on the plan it made
    plan.destroy()
    return False, ""


@pytest.mark.parametrize("name", sorted(D.FORMS))
def test_the_undamaged_file_loads_and_walks(E, O, name, tmp_path_factory):
    c, plan, f = form(E, O, name, tmp_path_factory)
    plan.check()
    assert D.strict_walk(f)
    path = tmp_path_factory.mktemp("again") / "p.ehyb"
    path.write_bytes(f.data)
    loaded, perm = E.Plan.load(path, key=c.m.key(), upload=False)
    assert np.array_equal(perm, c.perm)
    y, written = O.walk_plan(loaded, c.xp)
    assert written[:c.n].min() == 1 and c.check(y)[0] == 0
    # the strict walk can fail: a column of the residual, a halo column, a slab's first row, a unit's end outside their arrays
    s = f.scalars
    for arr, i, value, walked in (("er_col", 0, c.n, not s["er_panel"]), ("halo_cols", 0, -1, not s["direct"]),
                                  ("slab_meta", 2, -1, not s["direct"] and not s["sym"]), ("pb_units1", 3, len(f.a["pb_val"]) + 64, True), ("perm", 0, c.n, True)):
        if len(f.a[arr]) and walked:
            with pytest.raises(D.OutOfBounds):
                D.strict_walk(D.PlanFile(f.with_element(arr, i, value)))


@pytest.mark.parametrize("name", sorted(D.FORMS))
def test_targeted_mutations_are_refused(E, O, name, tmp_path_factory, tmp_path):
    c, plan, f = form(E, O, name, tmp_path_factory)
    tgt, _ = mutants(f, name)
    arrays = {arr for _, arr, _ in tgt}
    assert {n for n in D.INDEX_ARRAYS if len(f.a[n])} - {"slab_lrow"} <= arrays | {"ell_col"}, "an index array of the form without a targeted mutation"
    accepted = []
    for label, arr, data in tgt:
        (tmp_path / "m.ehyb").write_bytes(data)
        refused, why = load(E, tmp_path / "m.ehyb")
        if not refused:
            accepted.append(label)
    assert accepted == [], f"{name}: loaded although damaged: {accepted}"


@pytest.mark.parametrize("name", sorted(D.FORMS))
def test_random_mutants_are_refused_or_stay_in_bounds(E, O, name, tmp_path_factory, tmp_path):
    c, plan, f = form(E, O, name, tmp_path_factory)
    _, rnd = mutants(f, name)
    refused_of, unnamed, walked = {}, [], 0
    for label, arr, data in rnd:
        (tmp_path / "m.ehyb").write_bytes(data)
        refused, why = load(E, tmp_path / "m.ehyb")
        if refused:
            refused_of[arr] = refused_of.get(arr, 0) + 1
            if arr not in why.split("is damaged: ")[-1]:
                unnamed.append((label, why))
        else:
            try:
                D.strict_walk(D.PlanFile(data))      # accepted: it must address nothing out of bounds
            except D.OutOfBounds as e:
                raise AssertionError(f"{name}: {label} was accepted, and the strict walk leaves an array: {e}")
            walked += 1
    # not vacuous: per index array the form has, some random mutant was refused, and the refusals name the array
    have = [n for n in D.INDEX_ARRAYS if len(f.a[n])]
    assert [n for n in have if refused_of.get(n, 0) == 0] == [], (name, refused_of)
    assert unnamed == [], f"{name}: refusals that do not name the damaged array: {unnamed[:5]}"
    print(f"{name}: {sum(refused_of.values())} of {len(rnd)} random mutants refused, {walked} accepted and walked in bounds")


# ---------------------------------------------------------------------------------------------- 3. the load path under sanitizers
def test_load_path_under_host_sanitizers(E, O, tmp_path_factory, tmp_path):
    """csrc/plan_load_check.cpp, built with -fsanitize=address,undefined from the host sources alone, over every mutant above and
    the file cut at every array boundary, as a plain child process (the binary carries its sanitizer runtimes)."""
    csrc = os.path.join(ROOT, "ehyb_spmv_gpu_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "-j8", "-s", "plan_load_check"], capture_output=True, text=True)
    assert b.returncode == 0, "the sanitizer build of the load path failed (can this compiler link -fsanitize=address,undefined?):\n" + b.stdout + b.stderr
    exe = os.path.join(csrc, "build", "plan_load_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    for name in sorted(D.FORMS):
        c, plan, f = form(E, O, name, tmp_path_factory)
        tgt, rnd = mutants(f, name)
        files = [("undamaged", f.data)] + [(f"t{i}", d) for i, (_, _, d) in enumerate(tgt)] + [(f"r{i}", d) for i, (_, _, d) in enumerate(rnd)]
        files += [(f"cut{i}", d) for i, d in enumerate(f.truncations())]
        d = tmp_path / name
        d.mkdir()
        expect = {}
        for tag, data in files:
            p = d / f"{tag}.ehyb"
            p.write_bytes(data)
            expect[str(p)] = load(E, p)[0]
        assert not expect[str(d / "undamaged.ehyb")] and all(expect[str(d / f"cut{i}.ehyb")] for i in range(len(f.truncations())))
        r = subprocess.run([exe] + list(expect), capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, f"{name}: exit {r.returncode}\n{r.stderr[-4000:]}"
        got = {}
        for line in r.stdout.splitlines():
            path, verdict = line.split(" ")[:2]
            got[path] = verdict == "refused"
        assert got == expect, f"{name}: the program and the library disagree on {[os.path.basename(p) for p in expect if got.get(p) != expect[p]][:10]}"
        for p in expect:
            os.remove(p)
