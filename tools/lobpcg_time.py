#!/usr/bin/env python3
"""What ehyb_lobpcg costs on the audikw_1-like matrix made the M-matrix of tools/pcg_cheb_time.py (off-diagonals negative, diagonal =
row sum + shift * mean), with E.Coarse defaults and a plan that multiplies four columns per pass (cfg.lds_doubles =
EHYB_LDS_MAX_DOUBLES / 4): an iteration at nb = na = 4 split into its parts, and a solve end to end against ehyb_eigsh.

Per iteration, each part alone between HIP events on the tool's stream, the smallest of --rounds:
    multiply    ehyb_spmm of 4 columns
    gram        ehyb_lobpcg_gram_step at mc = 12 ([X | P | W], 24 columns read)
    rotation    ehyb_eigsh_rotate_step twice at (mc, kc) = (12, 8)
    residual    ehyb_lobpcg_resid_step for 4 columns, R into scratch columns, and ehyb_coarse_apply four times
    (beside them: the second launch of the residual step that a solve WITHOUT a coarse object makes once a column has converged,
    to pack W -- 3 of 4 columns active, inv_diag; it is no part of the iteration timed here)
    host        the wall time of a solve of 3 x --iters iterations (tol = 0) less that of --iters, over the 2 x --iters between
                them (the start and the staging through the host cancel), less the four parts: the two looks, the Rayleigh-Ritz
                step on the host, the uploads, the launches and the small sums
The columns hold random numbers: the kernels' work does not depend on the values.

End to end.  nev = 4 to tol 1e-8 with the two-level preconditioner against Plan.eigsh(4, "SA") in the same run: multiplies (columns
multiplied), iterations or restarts, the wall time around the call (best of --rounds; it includes staging the vectors through the
host), the true residual of every pair recomputed on the CPU.

--mass lumped, --mass consistent (or both words): ehyb_lobpcg_gen beside ehyb_lobpcg IN THE SAME RUN, on the same four-wide plan.  The
mass matrix has the bench matrix's pattern: m_ij = |k_ij| / s off the diagonal, m_ii = (2 sum_j |k_ij| + 0.01 s) / s with s the mean
off-diagonal row sum -- positive, strictly diagonally dominant, of order one --, put on K's partitions by Matrix.reorder_like with a
four-wide plan of its own; the lumped mass is its row sums.  Per form: the Gram kernel alone (ehyb_lobpcg_gram_b_step at mc = 12,
its bytes and TB/s), the microseconds of an iteration of a solve (as above), and nev = 4 to 1e-8 with the two-level preconditioner
(iterations, multiplies, wall ms, the true residual ||K x - theta M x|| recomputed on the CPU).  With a mass the lines go to
profiles/lobpcg_gen_time_audikw.jsonl.

usage: python tools/lobpcg_time.py [--workload audikw_1-like] [--shift 1e-2] [--sym 0] [--rounds 3] [--iters 20]
                                   [--mass {none,lumped,consistent} ...] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cg_multi_time import hip_events  # noqa: E402

LDS_MAX_DOUBLES = 20480
SCRATCH_DOUBLES = 294912


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--shift", type=float, default=1e-2)
    ap.add_argument("--sym", type=int, default=0, help="cfg.sym_pairs of the plan")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mass", nargs="+", choices=["none", "lumped", "consistent"], default=["none"],
                    help="also time ehyb_lobpcg_gen with this form of mass matrix (both forms may be named)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    forms = [f for f in ("lumped", "consistent") if f in args.mass]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lobpcg_gen_time_audikw.jsonl" if forms else "lobpcg_time_audikw.jsonl")
    import scipy.sparse as sp

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from ehyb_spmv_gpu_amd import _lib

    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()
    vp = C.c_void_p
    lib = _lib.load()

    def ok(rc):
        assert rc == 0, lib.ehyb_last_error()

    def timed_us(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        fn()
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value * 1e3

    def best_us(fn):
        fn()
        return min(timed_us(fn) for _ in range(args.rounds + 2))

    gen, gargs, _ = B.WORKLOADS[args.workload]
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=args.sym, lds_doubles=LDS_MAX_DOUBLES // 4)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I != J] = -np.abs(V[I != J])
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + args.shift * off.mean())[I[I == J]]
    mass_plan = lumped = Mp = None
    if forms:                                                    # the mass matrix in the original numbering, on K's pattern
        scale = off.mean()
        Vm = np.abs(V) / scale
        Vm[I == J] = ((2.0 * off + 0.01 * scale) / scale)[I[I == J]]
        rp0, J0 = m.row_idx.astype(np.int64), m.J.copy()
        lumped0 = np.bincount(I, weights=Vm, minlength=m.n)
    m.reorder(cfg)
    n = m.n
    if forms:
        mm = E.Matrix.from_csr(rp0, J0, Vm, cfg).reorder_like(m)
        del rp0, J0, Vm
        lumped = E.vector_reorder(lumped0, m.reorder_list)
        if "consistent" in forms:
            Mp = sp.csr_matrix((mm.V.copy(), mm.J.copy(), mm.row_idx.astype(np.int64)), shape=(n, n))
            mass_plan = E.Plan(mm, E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=2, lds_doubles=LDS_MAX_DOUBLES // 4))
        mm.free()
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))      # the permuted numbering, for the CPU checks
    plan = E.Plan(m, cfg)
    coarse = E.Coarse(m)
    print(f"# {args.workload}: n={n} nnz={m.nnz} sym_pairs={plan.stats['sym_pairs']} spmm_max_k={plan.spmm_max_k} coarse unknowns={coarse.nc}",
          flush=True)
    m.free()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    # ---------------------------------------------------------------- the parts of an iteration at nb = na = 4
    nb, mc = 4, 12
    ld = n + (n & 1)
    rng = np.random.default_rng(1)
    dS, dAS, dS2, dR = (E.DeviceBuffer(ld * mc) for _ in range(4))
    column = np.zeros(ld)
    for buf in (dS, dAS):
        for c in range(mc):                                      # one column at a time: no second copy of the basis on the host
            column[:n] = rng.standard_normal(n) / np.sqrt(n)
            ok(lib.ehyb_h2d(vp(buf.ptr + 8 * ld * c), column.ctypes.data_as(vp), column.nbytes))
    d = A.diagonal()
    dd = E.DeviceBuffer(n).upload(1.0 / d)
    dG, dH, dY, dth, dr2 = (E.DeviceBuffer(k) for k in (mc * mc, mc * mc, mc * 2 * nb, 8, 8))
    dY.upload(np.linalg.qr(rng.standard_normal((mc, mc)))[0][:, :2 * nb].T.ravel().copy())
    dth.upload(np.arange(1.0, 9.0))
    dscr, dpart = E.DeviceBuffer(SCRATCH_DOUBLES), E.DeviceBuffer(4096)
    s_ = vp(st.ptr)

    def multiply():
        plan.spmm(dS.ptr + 8 * ld * 2 * nb, dAS.ptr + 8 * ld * 2 * nb, nb, ldx=ld, ldy=ld, stream=st.ptr)

    def gram():
        ok(lib.ehyb_lobpcg_gram_step(n, ld, vp(dS.ptr), vp(dAS.ptr), mc, vp(dG.ptr), vp(dH.ptr), vp(dscr.ptr), s_))

    def rotation():
        ok(lib.ehyb_eigsh_rotate_step(n, ld, vp(dS.ptr), ld, vp(dS2.ptr), vp(dY.ptr), mc, 2 * nb, s_))
        ok(lib.ehyb_eigsh_rotate_step(n, ld, vp(dAS.ptr), ld, vp(dS2.ptr), vp(dY.ptr), mc, 2 * nb, s_))

    def residual():
        ok(lib.ehyb_lobpcg_resid_step(n, ld, vp(dS.ptr), vp(dAS.ptr), nb, vp(dth.ptr), None, (1 << nb) - 1, ld, vp(dR.ptr), vp(dr2.ptr),
                                      vp(dpart.ptr), s_))
        for c in range(nb):
            ok(lib.ehyb_coarse_apply(coarse.h, vp(dd.ptr), vp(dR.ptr + 8 * ld * c), vp(dS2.ptr + 8 * ld * c), s_))

    def packed():                                                # what a solve with Jacobi alone adds once a column has converged
        ok(lib.ehyb_lobpcg_resid_step(n, ld, vp(dS.ptr), vp(dAS.ptr), nb, vp(dth.ptr), vp(dd.ptr), 0b0111, ld, vp(dS2.ptr), vp(dr2.ptr),
                                      vp(dpart.ptr), s_))

    us_packed = best_us(packed)
    parts = {name: best_us(fn) for name, fn in (("multiply", multiply), ("gram", gram), ("rotation", rotation), ("residual", residual))}
    gram_b = {}
    for form in forms:                                           # the Gram kernel with the third image, alone
        third = E.DeviceBuffer(ld * mc if form == "consistent" else ld)
        if form == "consistent":
            for c in range(mc):
                column[:n] = rng.standard_normal(n) / np.sqrt(n)
                ok(lib.ehyb_h2d(vp(third.ptr + 8 * ld * c), column.ctypes.data_as(vp), column.nbytes))
        else:
            third.upload(np.concatenate([lumped, np.zeros(ld - n)]))
        bs, md = (vp(third.ptr), None) if form == "consistent" else (None, vp(third.ptr))
        us = best_us(lambda: ok(lib.ehyb_lobpcg_gram_b_step(n, ld, vp(dS.ptr), vp(dAS.ptr), bs, md, mc, vp(dG.ptr), vp(dH.ptr), vp(dscr.ptr), s_)))
        nbytes = 8 * n * (3 * mc if form == "consistent" else 2 * mc + 1)
        gram_b[form] = dict(us_gram_b=round(us, 1), MB_gram_b=round(nbytes / 1e6, 1), gram_b_TBps=round(nbytes / us / 1e6, 3))
        third.free()
    for b in (dS, dAS, dS2, dR, dG, dH, dY, dth, dr2, dscr, dpart, dd):
        b.free()

    def mass_of(form):
        return mass_plan if form == "consistent" else lumped

    def solve_us(iters, form=None):
        best = None
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            if form is None:
                info = plan.lobpcg(nb, coarse=coarse, inv_diag=1.0 / d, max_iter=iters, tol=0.0, vectors=False, stream=st.ptr)[2]
            else:
                info = plan.lobpcg_gen(nb, mass_of(form), coarse=coarse, inv_diag=1.0 / d, max_iter=iters, tol=0.0, vectors=False,
                                       stream=st.ptr)[2]
            t = (time.perf_counter() - t0) * 1e6
            best = t if best is None else min(best, t)
        assert info["iters"] == iters and info["multiplies"] == nb * (iters + 1), info
        return best

    per_iter = (solve_us(3 * args.iters) - solve_us(args.iters)) / (2 * args.iters)      # the start and the staging cancel
    per_iter_gen = {form: (solve_us(3 * args.iters, form) - solve_us(args.iters, form)) / (2 * args.iters) for form in forms}
    emit(dict(workload=args.workload, kind="iteration", n=n, nb=nb, na=nb, mc=mc, spmm_max_k=plan.spmm_max_k, sym_pairs=plan.stats["sym_pairs"],
              coarse_unknowns=coarse.nc, us_multiply=round(parts["multiply"], 1), us_gram=round(parts["gram"], 1),
              us_rotation=round(parts["rotation"], 1), us_residual_with_preconditioner=round(parts["residual"], 1),
              us_second_residual_launch_jacobi_3_of_4_active=round(us_packed, 1), us_host_and_rest=round(per_iter - sum(parts.values()), 1), us_per_iteration_of_a_solve=round(per_iter, 1),
              per_iteration_from=f"the wall time of {3 * args.iters} iterations less that of {args.iters}",
              MB_gram=round(8 * n * 2 * mc / 1e6, 1), gram_GBps=round(8 * n * 2 * mc / parts["gram"] / 1e3, 1)))

    for form in forms:
        emit(dict(workload=args.workload, kind="iteration_gen", mass=form, n=n, nb=nb, na=nb, mc=mc, spmm_max_k=plan.spmm_max_k,
                  mass_spmm_max_k=mass_plan.spmm_max_k if form == "consistent" else None,
                  us_per_iteration_of_a_solve=round(per_iter_gen[form], 1), us_per_iteration_of_ehyb_lobpcg_same_run=round(per_iter, 1),
                  over_ehyb_lobpcg=round(per_iter_gen[form] / per_iter, 3), us_gram_of_ehyb_lobpcg_same_run=round(parts["gram"], 1),
                  **gram_b[form]))

    # ---------------------------------------------------------------- end to end
    def solve(name, fn, count, Mh=None):
        wall, got = None, None
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            got = fn()
            ms = (time.perf_counter() - t0) * 1e3
            wall = ms if wall is None else min(wall, ms)
        ev, X, info = got
        nrm = float(np.abs(ev).max()) if len(ev) else 1.0
        mx = (lambda x: x) if Mh is None else (lambda x: Mh * x) if np.ndim(Mh) == 1 else (lambda x: Mh @ x)
        true = max((float(np.linalg.norm(A @ X[i] - ev[i] * mx(X[i]))) for i in range(len(ev))), default=0.0) / nrm
        emit(dict(workload=args.workload, kind="solve", solver=name, nev=4, tol=1e-8, nconv=info["nconv"], multiplies=info["multiplies"],
                  **{count: info[count]}, wall_ms=round(wall, 2), wall_includes="staging the vectors through the host",
                  evals=[float(f"{v:.12g}") for v in ev], true_residual_over_nrm=float(f"{true:.3e}")))

    solve("lobpcg, two-level preconditioner", lambda: plan.lobpcg(4, coarse=coarse, inv_diag=1.0 / d, tol=1e-8, stream=st.ptr), "iters")
    for form in forms:
        solve(f"lobpcg_gen, {form} mass, two-level preconditioner",
              lambda: plan.lobpcg_gen(4, mass_of(form), coarse=coarse, inv_diag=1.0 / d, tol=1e-8, stream=st.ptr), "iters",
              Mh=Mp if form == "consistent" else lumped)
    if not forms:
        solve("eigsh SA", lambda: plan.eigsh(4, "SA", tol=1e-8, stream=st.ptr), "restarts")
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
