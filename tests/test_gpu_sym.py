"""GPU parity of symmetric pair storage (cfg.sym_pairs = 1): an in-partition pair a_ij == a_ji is
stored once; the owning lane adds a_ij * x_j to its own row and a_ij * x_i to row j's accumulator in
LDS (ds_add_f64).  Same tolerance as every other path; the order of the LDS adds is not fixed, so
two runs may differ in the last bits -- by far less than the tolerance."""
import numpy as np
import pytest

from util import Case

pytestmark = pytest.mark.gpu

CASES = [
    ("fem3d-3dof", "fem3d", (30000, 3, 22, 22, 13500, 1, 1)),      # symmetric, shared column lists
    ("fem3d-1dof", "fem3d", (20000, 1, 30, 30, 50000, 1, 2)),
    ("fem3d-2dof", "fem3d", (20000, 2, 25, 25, 30000, 1, 3)),      # groups of two: the lane sums take one neighbour
    ("fem3d-6dof", "fem3d", (30000, 6, 18, 18, 13500, 1, 4)),      # groups of six: cut into two sums of three
    ("stencil", "stencil2d", (150, 150, 9, 3000, 1)),               # symmetric, short rows
    ("kkt", "kkt3d", (18,)),                                        # symmetric saddle point, zero diagonal block
    ("rmat", "rmat", (13, 1 << 16, 9)),                             # unsymmetric: almost nothing pairs up
]


@pytest.mark.parametrize("name,kind,args", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("lds,threads", [(2048, 256), (6144, 1024), (20480, 512)])
def test_sym_matches_oracle(E, O, gpu, name, kind, args, lds, threads):
    cfg = E.make_config(lds_doubles=lds, threads=threads, sym_pairs=1)
    c = Case(E, O, kind, args, cfg)
    plan = E.Plan(c.m, cfg)
    st = plan.stats
    assert st["nnz_ell"] + st["nnz_er"] == c.nnz
    if name != "rmat":
        assert st["sym_pairs"] > 0.2 * c.nnz
    y1 = plan.spmv_host(c.xp, iters=2)
    bad, worst = c.check(y1)
    assert bad == 0, f"{name} lds={lds}: {bad} rows over tolerance, worst {worst:.3e}"
    y2 = plan.spmv_host(c.xp)
    assert np.max(np.abs(y1 - y2)) <= 1e-13 * c.scale.max()      # run-to-run: last bits only
    # two-phase call (what a multi-GPU caller would use) agrees as well
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
    plan.spmv(dx.ptr, dy.ptr, phase=1)
    plan.spmv(dx.ptr, dy.ptr, phase=2)
    assert c.check(dy.download())[0] == 0


def test_sym_full_size_audikw_like(E, O, gpu):
    """BASELINE config 2 in full with symmetric pair storage: 256 partitions of at most 1.03 x the mean, one workgroup (and CU) each."""
    cfg = E.make_config(sym_pairs=1, value_map=1)
    c = Case(E, O, "fem3d", (943695, 3, 68, 68, 13500, 1, 1), cfg)
    plan = E.Plan(c.m, cfg)
    st = plan.stats
    # 256 partitions asked for, one workgroup each; the partitioner may leave a few of them empty (its balance
    # constraint is an upper bound: 3 % above the mean), and an empty partition has no work item
    assert 248 <= st["n_parts"] <= 256 and st["n_items"] == st["n_parts"]
    assert st["sym_pairs"] > 0.35 * c.nnz and st["size_block_ell"] < 0.68 * c.nnz
    y = plan.spmv_host(c.xp)
    bad, worst = c.check(y)
    assert bad == 0, f"worst {worst:.3e}"
    # checksum of checksums: sum_i y_i == sum_j (column sum_j) x_j
    colsum = np.zeros(c.n)
    np.add.at(colsum, c.m.J, c.m.V)
    assert abs(y.sum() - float(colsum @ c.xp)) <= 1e-11 * float(np.abs(c.m.V).sum())
    # the numeric phase on the device at full size (ehyb_plan_set_values): A -> -3 A + sign pattern kept symmetric;
    # scaling by a power of two times three is not exact, so the refilled plan is compared with the oracle's y on
    # the new values, which for V' = -3 V is -3 y_ref up to the rounding of the products
    plan.set_values(-3.0 * c.m.V)
    y3 = plan.spmv_host(c.xp)
    bad, worst = O.check_strict(c.recover(y3), -3.0 * c.y_ref, 3.0 * c.scale)
    assert bad == 0, f"after the refill: worst {worst:.3e}"
    plan.set_values(c.m.V)                       # and back: the original product again
    assert c.check(plan.spmv_host(c.xp))[0] == 0
