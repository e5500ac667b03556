"""The fuzz cases of test_fuzz_layout.py in exact mode (exact_cases.py): integer values and x, so that the product is
one number in fp64 whatever the order of summation.  Every layout is walked the way the kernels index it
(oracle.walk_plan) and must give that number bit for bit, every row written once -- an entry counted twice, dropped,
or added to the wrong row shows here, below the tolerance the float cases allow, before any GPU time is spent."""
import numpy as np
import pytest

from exact_cases import assert_exact
from fuzz_cases import build


@pytest.mark.parametrize("seed", range(48))
def test_exact_layout_walk(E, O, seed):
    m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True)
    plan = E.Plan(m, cfg, upload=False)
    yp, written = O.walk_plan(plan, E.vector_reorder(x, m.reorder_list))
    assert (written == 1).all(), kw
    assert_exact(E.vector_recover(yp, m.reorder_list), y_ref, str(kw))
    st = plan.stats
    assert st["nnz_ell"] + st["nnz_er"] == m.nnz, kw


def test_exact_mode_pairs_by_accident(E, O):
    """Small integer values give a matrix that is not symmetric entries a_ij == a_ji by accident: symmetric pair
    storage must meet such pairs among the fuzz seeds, or the seeds above would not exercise them."""
    found = 0
    for seed in range(48):
        m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True)
        A = m.to_scipy()
        if kw["sym_pairs"] == 1 and m.nnz and abs(A - A.T).nnz != 0:
            found += E.Plan(m, cfg, upload=False).stats["sym_pairs"] > 0
    assert found >= 1


@pytest.mark.parametrize("seed", range(200, 212))
def test_exact_plan_cache_round_trip(E, O, seed, tmp_path):
    """ehyb_plan_save / ehyb_plan_load in exact mode: the loaded plan walks to the same exact product."""
    m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True)
    plan = E.Plan(m, cfg, upload=False)
    path = tmp_path / "p.cache"
    plan.save(path, reorder_list=m.reorder_list, key=777)
    back, perm = E.Plan.load(path, key=777, upload=False)
    assert np.array_equal(perm, m.reorder_list), kw
    for name in ("ell_val", "er_val", "pb_val"):
        assert np.array_equal(plan.array(name), back.array(name)), (name, kw)
    yp, written = O.walk_plan(back, E.vector_reorder(x, perm))
    assert (written == 1).all(), kw
    assert_exact(E.vector_recover(yp, perm), y_ref, str(kw))
