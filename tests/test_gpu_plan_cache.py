"""A plan that came from a cache file through EVERY entry point a loaded plan can be given to, on the device, next to the plan it
was saved from: ehyb_spmv, its two phases, both explicit walks, ehyb_spmm at every width the plan serves, ehyb_spmv_t where the
form is served, the multiply in parts of a column-segment plan.  One small plan per form (plan_damage.FORMS, a few thousand
rows); undamaged files only -- what a damaged file does is the CPU's business (test_plan_check.py).

Both plans must agree with the CPU oracle under the strict check; where the multiply is deterministic -- plain storage, no
panel-form residual (the rule of test_gpu_set_values.py: LDS atomics add in any order) -- they must agree with each other bit
for bit.  The rows of a CSR residual that are split into several segments are added with one fp64 atomic per segment
(ell_device.h er_bin), in any order: on those rows alone the bitwise comparison gives way to the strict check.  The transposed
multiply is atomic adds throughout and is held to the strict check.  The loaded plan must launch the very kernels the original
launches (ehyb_debug_launched), and report the same widths, support, stats and resident bytes."""
import numpy as np
import pytest

import plan_damage as D

pytestmark = pytest.mark.gpu


def _pair(E, O, name, tmp_path):
    c, plan, col_segs = D.build_form(E, O, name)          # ell_keep, ell_triples, value_map at their defaults, as a loaded plan has them
    path = tmp_path / "plan.ehyb"
    plan.save(path, c.perm, key=c.m.key())
    loaded, perm = E.Plan.load(path, key=c.m.key(), upload=True)
    plan.upload()
    assert np.array_equal(perm, c.perm)
    return c, plan, loaded


class _Ops:
    """runs one operation on both plans with the same input and compares"""

    def __init__(self, E, O, c, plan, loaded, name):
        self.E, self.O, self.c, self.plans, self.name = E, O, c, (plan, loaded), name
        m = c.m
        self.n = m.n
        self.I, self.J = m.I.copy(), m.J.copy()
        V = m.V.copy()
        self.V = V.astype(np.float32).astype(np.float64) if name == "val-f32" else V      # the values as the device holds them
        st = plan.stats
        self.deterministic = st["sym_pairs"] == 0 and st["er_partials"] == 0
        rows = plan.array("er_seg_row")
        self.split = np.unique(rows[rows < 0] & 0x7FFFFFFF)                               # rows added with one atomic per segment
        self.lib = E.host._lib.load()

    def reference(self, x, transposed=False):
        I, J = (self.J, self.I) if transposed else (self.I, self.J)
        return self.O.spmv_coo(self.n, I, J, self.V, x), self.O.abs_rowsum(self.n, I, J, self.V, x)

    def run(self, what, call, X, k=1, transposed=False):
        """call(plan, dx, dy) on both plans; X: [k][n] in the plan's numbering"""
        outs = []
        for plan in self.plans:
            dx, dy = self.E.DeviceBuffer(self.n * k).upload(X.reshape(-1)), self.E.DeviceBuffer(self.n * k)
            dy.upload(np.full(self.n * k, np.nan))
            call(plan, dx, dy)
            assert self.lib.ehyb_dev_sync() == 0
            outs.append(dy.download().reshape(k, self.n))
            dx.free(), dy.free()
        for j in range(k):
            y_ref, scale = self.reference(X[j], transposed)
            for who, out in zip(("original", "loaded"), outs):
                bad, worst = self.O.check_strict(out[j], y_ref, scale)
                assert bad == 0, f"{self.name} {what} column {j}, {who} plan: {bad} rows differ from the oracle (worst {worst:.3e})"
        if self.deterministic and not transposed:
            a, b = outs[0].copy(), outs[1].copy()
            a[:, self.split] = b[:, self.split] = 0.0
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"{self.name} {what}: the loaded plan differs bitwise from the original"


@pytest.mark.parametrize("name", sorted(D.FORMS))
def test_loaded_plan_through_every_entry_point(E, O, gpu, name, tmp_path):
    c, plan, loaded = _pair(E, O, name, tmp_path)
    ops = _Ops(E, O, c, plan, loaded, name)
    st = plan.stats
    n = c.n
    x = c.xp
    X = np.stack([np.roll(x, 7 * j) * (1.0 + 0.25 * j) for j in range(4)])
    # what needs no launch agrees
    assert loaded.stats == st and loaded.spmm_max_k == plan.spmm_max_k and loaded.spmv_t_supported == plan.spmv_t_supported
    assert loaded.resident_bytes == plan.resident_bytes and loaded.col_segs == plan.col_segs
    assert loaded.launched() == plan.launched() == dict(window=set(), panel=set(), er_csr=set())
    ops.run("ehyb_spmv", lambda p, dx, dy: p.spmv(dx.ptr, dy.ptr), X[:1])
    assert c.n <= 6000 and c.nnz <= 400000          # (small: none is a benchmark matrix)
    direct = name == "direct"
    if not direct:      # (the direct shape is one launch: it has no phases)

        def phases(p, dx, dy):
            p.spmv(dx.ptr, dy.ptr, phase=1)
            p.spmv(dx.ptr, dy.ptr, phase=2)

        ops.run("ehyb_spmv_phase 1, 2", phases, X[1:2])
    else:
        for p in (plan, loaded):
            with pytest.raises(E.EhybError) as e:
                p.spmv(0x1000, 0x1000, phase=1)
            assert e.value.code == 8
    for walk in (0, 1):
        ops.run(f"ehyb_spmv_walk {walk}", lambda p, dx, dy: p.spmv(dx.ptr, dy.ptr, walk=walk), X[2:3])
    kmax = plan.spmm_max_k
    assert (kmax == 1) == (name == "val-f32"), (name, kmax)     # (the fp32-value kernels are one column wide; the others serve several)
    for k in range(2, kmax + 1):
        for walk in (None, 1):
            ops.run(f"ehyb_spmm k={k} walk={walk}", lambda p, dx, dy: p.spmm(dx.ptr, dy.ptr, k, walk=walk), X[:k], k=k)
    if plan.spmv_t_supported:
        ops.run("ehyb_spmv_t", lambda p, dx, dy: p.spmv_t(dx.ptr, dy.ptr), X[3:4], transposed=True)
        assert loaded.launched_t() == plan.launched_t() != set()
    else:
        assert loaded.spmv_t_refusal == plan.spmv_t_refusal
    if name == "column-segments":
        # the parts in the order a rank issues them (test_gpu_parts.py): own columns first, then segment by segment, the closing pass last
        def parts(p, dx, dy):
            p.spmv_part(dx.ptr, dy.ptr, 0, 0, 1, 1)
            p.spmv_part(dx.ptr, dy.ptr, 0, 1, 3, 0)
            p.spmv_part(dx.ptr, dy.ptr, 0, 3, 4, 2)

        assert plan.col_segs == 4
        ops.run("ehyb_spmv_part", parts, X[1:2])
    # the same calls launched the same kernels
    assert loaded.launched() == plan.launched(), name
    assert any(loaded.launched().values())
    # a loaded plan holds no slot maps: it cannot be refilled
    with pytest.raises(E.EhybError) as e:
        loaded.set_values(c.m.V.copy())
    assert e.value.code == 8
    loaded.destroy(), plan.destroy()
