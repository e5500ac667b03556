"""CPU walk of the TRANSPOSED multiply over a plan's host arrays, indexing them as ehyb_ell_t_kernel / ehyb_er_t_kernel do
(csrc/ell_t_device.h): per segment a window of accumulators -- own columns from the even row at or below the partition start,
then the halo columns --, every lane's value * x[row] added to the window column of its entry, and the flush that leaves out
acc[0] of an odd-start partition.  Checks the scheme and the flush rule without a GPU, over the host's column words (pair form)
or over the words and slab records as ehyb_plan_upload sends them (device=True: triple-coded where cfg.ell_triples codes a slab,
decoded as the kernel's triple arm does -- three pairs per word, then a word for one or two).  No tests here (test_spmv_t_host.py)."""
import numpy as np

from test_col_triples import device_cols


def _triple_columns(words, c0, npairs, G, groups):
    """[pair][lane][half] columns of a triple-coded slab, walked as ell_slab_t walks it"""
    c = np.zeros((npairs, 64, 2), dtype=np.int64)
    left, k, at = npairs, 0, c0
    while left > 0:
        w = words[at:at + G][groups]
        a, b = w & 0xFFFF, w >> 16
        for q, (lo, hi) in enumerate(((a, a + 1), (a + 2, b), (b + 1, b + 2))[:min(left, 3)]):
            c[k + q, :, 0], c[k + q, :, 1] = lo, hi
        k, left, at = k + 3, left - 3, at + G
    return c


def walk_plan_t(plan, x, device=False):
    """-> y = A^T x (permuted numbering) for a plan ehyb_spmv_t serves"""
    x = np.asarray(x, dtype=np.float64)
    n = plan.n
    y = np.zeros(n)
    halo_cols = plan.array("halo_cols")
    ell_val = plan.array("ell_val")
    ell_col = plan.array("ell_col").astype(np.int64)
    lane_group = plan.array("lane_group").astype(np.int64).reshape(-1, 64) & 0x3F
    meta = plan.array("slab_meta").astype(np.int64).reshape(-1, 4)
    if device:
        ell_col, meta = device_cols(plan)
        ell_col, meta = ell_col.astype(np.int64), meta.astype(np.int64)
    items = plan.array("items").reshape(-1, 8)
    segs = plan.array("segs").reshape(-1, 8)
    st = plan.stats
    direct = st["nnz_ell"] == 0 and st["nnz_er"] == st["nnz"] and st["er_segments"] == n
    inline = st["er_inline"] > 0
    lanes = np.arange(64)
    for g0, g1 in (items[:, :2] if not direct else ()):
        for g in range(g0, g1):
            p, s0, s1, hn, ps, pe, wl, hb = (int(v) for v in segs[g])
            if wl == 0 and hn == 0:
                continue
            base, cnt = ps & ~1, wl + (ps & 1)
            acc = np.zeros(cnt + hn)
            for s in range(s0, s1):
                p0, c0, r0, shape = (int(v) for v in meta[s])
                npairs, ner, G = shape >> 16, (shape >> 8) & 0xFF, (shape & 0x3F) + 1
                has = r0 + lanes < pe
                xi = np.where(has, x[np.minimum(r0 + lanes, n - 1)], 0.0)
                if npairs:
                    v = ell_val[p0 * 128:(p0 + npairs) * 128].reshape(npairs, 64, 2)
                    if shape & 0x40:
                        assert device and not shape & 0x80 and not ner
                        c = _triple_columns(ell_col, c0, npairs, G, lane_group[s])
                    else:
                        words = ell_col[c0:c0 + npairs * G].reshape(npairs, G)[:, lane_group[s]]
                        c = np.stack([words & 0xFFFF, words >> 16], axis=2)
                    if shape & 0x80:
                        c = (c + (r0 + lanes - base)[None, :, None]) & 0xFFFF
                    hv = np.broadcast_to(has[None, :, None], c.shape)
                    assert c[hv].max() < cnt + hn, "window column outside the window"
                    np.add.at(acc, c[hv], (v * xi[None, :, None])[hv])
                if ner:
                    assert inline
                    ve = ell_val[(p0 + npairs) * 128:(p0 + npairs + ner) * 128].reshape(ner, 64, 2)
                    ce = ell_col[c0 + npairs * G:c0 + npairs * G + ner * 128].reshape(ner, 2, 64).transpose(0, 2, 1)
                    hv = np.broadcast_to(has[None, :, None], ce.shape)
                    np.add.at(y, ce[hv], (ve * xi[None, :, None])[hv])
            lo = ps & 1                                        # acc[0] of an odd-start partition is row ps - 1: never flushed
            np.add.at(y, base + np.arange(lo, cnt), acc[lo:cnt])
            np.add.at(y, halo_cols[hb:hb + hn], acc[cnt:])
    if not inline:
        seg_ptr, seg_row = plan.array("er_seg_ptr"), plan.array("er_seg_row")
        if len(seg_row):
            rows = np.repeat(seg_row & 0x7FFFFFFF, np.diff(seg_ptr))
            np.add.at(y, plan.array("er_col"), plan.array("er_val") * x[rows])
    return y
