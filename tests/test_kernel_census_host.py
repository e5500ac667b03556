"""The kernel census on the CPU (kernel_census_cases.py): the rows the cases declare ARE the rows of the library's three kernel
tables -- an instantiation added to a table without a case that launches it fails here --, and every case's host-only plan is the
plan the case claims: path taken, slabs against waves, halo, segments per item, ehyb_spmm_max_k.  No GPU compute is called."""
import pytest

from kernel_census_cases import CASES, ELSEWHERE, EXEMPT, SHOWS, THREADS, build_matrix, check_plan, f32_window_row

TABLE_ROWS = {"window": 96, "panel": 22, "er_csr": 10}


def test_tables_need_no_device_and_have_the_documented_rows(E):
    for name, fields in E.KERNEL_TABLES.items():
        rows = E.kernel_table(name)
        assert len(rows) == TABLE_ROWS[name] == len(set(rows)), (name, len(rows))
        assert all(len(r) == len(fields) for r in rows)
    win = E.kernel_table("window")
    f = E.KERNEL_TABLES["window"]
    assert f == ("threads", "k", "dyn", "stamp", "inl", "sym", "f32")
    assert {r[0] for r in win} == set(THREADS) and {r[1] for r in win} == {1, 2, 3, 4}
    # the static walk and the stamps are one vector wide and fp64; fp32 is one vector wide with the LDS counter
    assert all(r[1] == 1 and r[6] == 0 for r in win if r[2] == 0 or r[3] == 1)
    assert all(r[1] == 1 and r[2] == 1 and r[3] == 0 for r in win if r[6] == 1)
    # a bad table, and a buffer that holds fewer rows than the table
    import ctypes as C

    lib = E.host._lib.load()
    n = C.c_int(-1)
    assert lib.ehyb_debug_kernel_table(3, None, 0, C.byref(n)) == 1
    few = (C.c_int32 * 14)(*([-7] * 14))
    assert lib.ehyb_debug_kernel_table(0, few, 1, C.byref(n)) == 0 and n.value == 96
    assert tuple(few[:7]) == win[0] and list(few[7:]) == [-7] * 7


@pytest.mark.parametrize("table", sorted(TABLE_ROWS))
def test_the_cases_cover_the_table(E, table):
    """union of the declared rows == the table's rows: no instantiation without a case, no case for a row that is not built"""
    declared = set().union(*(c.rows.get(table, set()) for c in CASES))
    declared |= {row for t, row, _ in ELSEWHERE if t == table}
    assert all(reason and "\n" not in reason for _, _, reason in EXEMPT)
    exempt = {row for t, row, _ in EXEMPT if t == table}
    built = set(E.kernel_table(table))
    assert not (declared & exempt), "an exempted row has a case"
    assert built - declared - exempt == set(), f"{table}: instantiations no case launches"
    assert declared | exempt == built, f"{table}: rows declared that the library does not build: {sorted((declared | exempt) - built)}"
    assert EXEMPT == []


def test_window_arm_of_val_f32_names_rows_of_the_table(E):
    win = set(E.kernel_table("window"))
    for threads in THREADS:
        for inl in (False, True):
            for sym in (False, True):
                assert f32_window_row((threads, inl, sym)) in win
    assert {row for t, row, _ in ELSEWHERE if t == "window"} == {r for r in win if r[6] == 1}


def test_every_walk_and_workgroup_size_can_go_wrong():
    """per walk (dyn) and workgroup size some case shows each of: more slabs than waves, fewer, a halo, several segments per item
    (what the cases CLAIM; test_host_plan_is_what_the_case_claims holds every case to its claim)"""
    for dyn in (0, 1):
        for threads in THREADS:
            for what in SHOWS:
                assert any(c.walk_key == (dyn, threads) and what in c.shows for c in CASES), (dyn, threads, what)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_host_plan_is_what_the_case_claims(E, case):
    cfg = case.cfg(E)
    plan = E.Plan(build_matrix(E, case), cfg, upload=False)
    check_plan(case, plan, int(cfg.threads))
    assert plan.launched() == dict(window=set(), panel=set(), er_csr=set())     # nothing was launched
    plan.destroy()
