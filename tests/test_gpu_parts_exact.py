"""The multiply in PARTS (include/ehyb.h "The multiply in PARTS": ehyb_spmv_part, ehyb_step_pack, ehyb_step_part, ehyb_halo_step),
pinned in one process, on the small rank-local matrices of parts_cases.py, bit for bit (exact_cases.py: integer values and x).

What the overlap of exchange and compute rests on is tested where it breaks deterministically: x on the device holds the own
columns and POISON in every ghost column; a chunk's true values are copied in only just before the part that may read them is
issued.  A part that reads a column that has not arrived, a pass 2 that covers the wrong row blocks, a middle part that writes y,
a partial sum that survives into the next step: each gives a wrong number, not a lost race.  y is filled with NaN before a step
unless a test says otherwise, every vector carries a pad of sentinels that must survive, the rows of y behind the plan's rows
must keep what they held, and x must come back as it was put.  test_parts_host.py proves, without a GPU, that the cases have
the panels, row blocks and windows these tests need."""
import ctypes as C

import numpy as np
import pytest

import parts_cases as PC
from exact_cases import assert_exact, integer_x
from parts_cases import PART_FIRST as FIRST, PART_LAST as LAST, PART_LAST_FOREIGN as LAST_FOREIGN
from solver_cases import PAD, SENTINEL

pytestmark = pytest.mark.gpu

POISONS = {"2^60": 2.0 ** 60, "nan": np.nan}   # 2^60: finite (a zero-valued padding slot that reads it adds 0), and no row that reads it
#                                                through a real entry (|a| >= 1, |y| < 2^52) can come out exact


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pattern(n, seed):
    """n doubles of arbitrary bits (NaN payloads included): what a launch that must not write y has to leave"""
    return np.random.default_rng(seed).integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64).view(np.float64)


@pytest.fixture(scope="module")
def plans(E, gpu):
    """the uploaded plan of every case, made when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            c = PC.case(E, name)
            made[name] = (c, c.plan())
        return made[name]

    yield get
    for _, plan in made.values():
        plan.destroy()


class Dev:
    """x and y of one case on the device, a pad behind each; the host keeps what it put there."""

    def __init__(self, E, c, x=None):
        self.E, self.c, self.lib = E, c, E.host._lib.load()
        self.x_true = c.x if x is None else x
        self.dx, self.dy = E.DeviceBuffer(c.n + PAD), E.DeviceBuffer(c.n + PAD)
        self.hx = np.full(c.n + PAD, SENTINEL)
        self.hy = np.full(c.n + PAD, SENTINEL)

    def put_x(self, poison=None):
        """the own columns true; the ghost columns POISON, or true as well (None)"""
        n0, n = self.c.n0, self.c.n
        self.hx[:n] = self.x_true
        if poison is not None:
            self.hx[n0:n] = poison
        self.dx.upload(self.hx)
        return self

    def deliver(self, c0, c1):
        """the true x of columns [c0, c1) arrives"""
        if c1 > c0:
            part = np.ascontiguousarray(self.x_true[c0:c1])
            assert self.lib.ehyb_h2d(C.c_void_p(self.dx.ptr + 8 * c0), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0
            self.hx[c0:c1] = part

    def forget(self, c0, c1, poison):
        """columns [c0, c1) of x hold POISON again: nobody may need them any more"""
        if c1 > c0:
            self.hx[c0:c1] = poison
            part = np.ascontiguousarray(self.hx[c0:c1])
            assert self.lib.ehyb_h2d(C.c_void_p(self.dx.ptr + 8 * c0), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0

    def put_y(self, fill=np.nan, rows=None):
        """y (all of it, or rows [r0, r1)) = fill: a number or an array"""
        r0, r1 = (0, self.c.n) if rows is None else rows
        self.hy[r0:r1] = fill
        if rows is None:
            r1 += PAD                                       # (the pad goes along)
        part = np.ascontiguousarray(self.hy[r0:r1])
        assert self.lib.ehyb_h2d(C.c_void_p(self.dy.ptr + 8 * r0), part.ctypes.data_as(C.c_void_p), part.nbytes) == 0
        return self

    def y(self, what):
        """synchronise -> the plan's rows of y; the rows behind them and the pad hold what they held, x and its pad what was put"""
        assert self.lib.ehyb_dev_sync() == 0, what
        y, x = self.dy.download(), self.dx.download()
        nr = self.c.n_rows
        assert np.array_equal(_bits(y[nr:]), _bits(self.hy[nr:])), f"{what}: y behind the plan's rows, or its pad, was written"
        assert np.array_equal(_bits(x), _bits(self.hx)), f"{what}: x or its pad was written"
        return y[:nr]

    def free(self):
        self.dx.free(), self.dy.free()


def rank_parts(c):
    """The parts in the order a rank issues them -> [(chunk to deliver first or None, seg_begin, seg_end, flags)]: own columns with
    FIRST (and the close of the foreign rows on the split plan), then chunk by chunk, LAST on the final one.  CSR form: the
    residual launch needs all of x, so FIRST, everything delivered, LAST."""
    if not c.panel:
        return [(None, 0, 1, FIRST), ("all", 1, c.n_segs, LAST)]
    parts = [(None, 0, 1, FIRST | (LAST_FOREIGN if c.split else 0))]
    for s, c0, c1 in c.chunks():
        parts.append(((c0, c1), s, s + 1, LAST if s == c.n_segs - 1 else 0))
    return parts


def issue(plan, d, parts, stream=0, after_first=None, forget=None):
    """forget = a POISON (panel form): once a part is enqueued the columns of its segments hold POISON again -- pass 1 "needs x of
    those columns only", so no later part may read them, and the closing pass reads no x at all"""
    for k, (arrive, s0, s1, flags) in enumerate(parts):
        if arrive == "all":
            d.deliver(d.c.n0, d.c.n)
        elif arrive is not None:
            d.deliver(*arrive)
        plan.spmv_part(d.dx.ptr, d.dy.ptr, stream, s0, s1, flags)
        if k == 0 and after_first is not None:
            after_first()
        if forget is not None and d.c.panel:
            d.forget(int(d.c.segs[s0]), int(d.c.segs[s1]), forget)


# ---------------------------------------------------------------------------------------------- parts read only what has arrived
@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("name,earlier", [(n, e) for n in PC.CASES for e in ("kept", "forgotten") if e == "kept" or n in PC.PANEL_CASES])
def test_parts_read_only_what_has_arrived(E, plans, name, poison, earlier):
    """Every ghost column holds POISON until just before the part that owns it is issued; the product is exact all the same.  On
    the plans with windows y after the FIRST part (+ segment 0's pass 1, which writes no y) is the exact sum of the window entries:
    finite, no trace of the poison.  The NaN run also pins that no zero-valued padding slot points outside the part's columns.
    earlier = kept: x fills up as on a rank; forgotten (panel form): the columns of a part are poisoned again behind it, the own
    columns included, so that at every part x holds that part's columns and nothing else (the CSR residual launch needs all of x)."""
    c, plan = plans(name)
    d = Dev(E, c).put_x(POISONS[poison]).put_y()
    plan.launched_clear()

    def after_first():
        if c.windows:
            yw, rows = c.window_product(plan, c.x)
            assert rows.all()
            assert_exact(d.y(f"{name} {poison} after FIRST"), yw, f"{name} poison {poison}: y after the FIRST part against the windows' exact sum")

    issue(plan, d, rank_parts(c), after_first=after_first, forget=POISONS[poison] if earlier == "forgotten" else None)
    assert_exact(d.y(f"{name} {poison}"), c.y_ref, f"{name} poison {poison}, earlier columns {earlier}: the whole step")
    # the kernels the case names were the ones launched
    ran = plan.launched()
    assert bool(ran["panel"]) == c.panel and bool(ran["er_csr"]) == (not c.panel) and bool(ran["window"]) == c.windows, (name, ran)
    if c.panel:
        assert {r[0] for r in ran["panel"]} == {1, 2}, "both passes"
    f32 = c.cfg.val_f32 == 1
    assert all(r[-1] == int(f32) for r in ran["window"] | ran["er_csr"]), (name, ran)
    d.free()


def test_val_f32_with_a_panel_residual_is_refused_at_upload(E, gpu):
    """cfg.val_f32 has no panel passes: the plan never reaches ehyb_spmv_part (csr-windows-f32 is the arm that multiplies)."""
    c = PC.case(E, "panel-all")
    cfg = E.make_config(n_top=2, val_f32=1, **PC.CASES["panel-all"][1], **PC.CASES["panel-all"][2])
    with pytest.raises(E.EhybError) as ei:
        E.Plan(c.m, cfg, rows=(0, c.n_rows), col_segs=c.segs)
    assert ei.value.code == PC.ERR_ARG and "cfg.val_f32 is not built for a residual in panel form" in str(ei.value)


# ---------------------------------------------------------------------------------------------- middle parts write no y
@pytest.mark.parametrize("name", PC.PANEL_CASES)
def test_middle_parts_write_no_y(E, plans, name):
    """A part without flags is pass 1 alone: it fills partial sums and leaves every bit of y."""
    c, plan = plans(name)
    d = Dev(E, c).put_x().put_y(_pattern(c.n, 3))
    for s0, s1 in [(s, s + 1) for s in range(c.n_segs)] + [(0, c.n_segs), (1, 3), (2, 2)]:
        plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, s0, s1, 0)
        assert np.array_equal(_bits(d.y(f"{name} [{s0},{s1})")), _bits(d.hy[:c.n_rows])), f"{name}: pass 1 of segments [{s0}, {s1}) wrote y"
    d.free()


@pytest.mark.parametrize("seg", [1, 2, 3, 4])
@pytest.mark.parametrize("name", PC.PANEL_CASES)
def test_a_middle_part_renews_its_own_partial_sums_only(E, plans, name, seg):
    """Pass 1 over everything with x, then -- x replaced by another vector altogether -- the part of ONE ghost chunk, then the closing
    pass alone: the product of a vector that holds the new values in that chunk's columns and the old ones everywhere else (the
    windows hold no ghost column: theirs were multiplied with the old x).  A part that walked more than its own panels shows."""
    c, plan = plans(name)
    n, x2 = c.n_segs, integer_x(c.n, 5)
    c0, c1 = int(c.segs[seg]), int(c.segs[seg + 1])
    mixed = c.x.copy()
    mixed[c0:c1] = x2[c0:c1]
    d = Dev(E, c).put_x().put_y()
    plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, 0, n, FIRST)
    d.x_true = x2
    d.put_x()
    plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, seg, seg + 1, 0)
    plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, n, n, LAST | (LAST_FOREIGN if c.split else 0))
    want = c.reference(mixed)
    assert (c1 == c0) == np.array_equal(want, c.y_ref), "the chunk's columns matter unless it is the empty one"
    assert_exact(d.y(f"{name} segment {seg}"), want, f"{name}: the part of segment {seg} alone between a whole pass 1 and the closing pass")
    d.free()


# ---------------------------------------------------------------------------------------------- foreign rows
@pytest.mark.parametrize("poison", list(POISONS))
def test_foreign_rows_close_early_and_stay_closed(E, plans, poison):
    c, plan = plans("panel-split")
    split, nr = c.n0, c.n_rows
    d = Dev(E, c).put_x(POISONS[poison]).put_y()
    parts = rank_parts(c)
    issue(plan, d, parts[:1])
    y = d.y("foreign close")
    assert_exact(y[split:], c.y_ref[split:], f"poison {poison}: the foreign rows after FIRST + segment 0 + LAST_FOREIGN")
    assert np.isnan(y[:split]).all(), "LAST_FOREIGN closed a row in front of cfg.row_split"
    d.put_y(SENTINEL, rows=(split, nr))
    issue(plan, d, parts[1:])
    y = d.y("own close")
    assert_exact(y[:split], c.y_ref[:split], f"poison {poison}: the own rows after LAST")
    assert np.array_equal(_bits(y[split:]), _bits(np.full(nr - split, SENTINEL))), "LAST wrote a row from cfg.row_split on"
    d.free()


def test_one_call_with_all_three_flags_is_ehyb_spmv(E, plans):
    c, plan = plans("panel-split")
    d, w = Dev(E, c).put_x().put_y(), Dev(E, c).put_x().put_y()
    plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, 0, c.n_segs, FIRST | LAST | LAST_FOREIGN)
    plan.spmv(w.dx.ptr, w.dy.ptr)
    y_parts, y_whole = d.y("one call"), w.y("ehyb_spmv")
    assert_exact(y_parts, c.y_ref, "one call, every segment, all three flags")
    assert_exact(y_whole, c.y_ref, "ehyb_spmv on the split plan")
    d.free(), w.free()


# ---------------------------------------------------------------------------------------------- any grouping
def groupings(c):
    """-> {name: [(seg_begin, seg_end, flags)]}; on the split plan the call that completes segment 0's pass 1 closes the foreign rows"""
    n, lf = c.n_segs, LAST_FOREIGN if c.split else 0
    one_each = [(s, s + 1, (FIRST | lf if s == 0 else 0) | (LAST if s == n - 1 else 0)) for s in range(n)]   # the empty segment a part of its own
    ranges = [(0, 2, FIRST | lf), (2, 2, 0), (2, n, LAST)]
    reversed_ = [(0, 0, FIRST)] + [(s, s + 1, 0) for s in reversed(range(n))] + [(0, 0, LAST | lf)]
    flags_apart = [(0, 0, FIRST), (0, n, 0), (n, n, lf), (n, n, LAST)]
    return {"one each": one_each, "ranges": ranges, "reversed": reversed_, "flags apart": flags_apart, "one call": [(0, n, FIRST | LAST | lf)]}


@pytest.mark.parametrize("name", list(PC.CASES))
def test_any_grouping_of_segments(E, plans, name):
    c, plan = plans(name)
    d = Dev(E, c).put_x()
    for what, calls in groupings(c).items():
        d.put_y()
        for s0, s1, flags in calls:
            plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, s0, s1, flags)
        assert_exact(d.y(f"{name} {what}"), c.y_ref, f"{name}, segments {what}")
    d.free()


# ---------------------------------------------------------------------------------------------- two steps
@pytest.mark.parametrize("name", list(PC.CASES))
def test_two_steps_with_different_x(E, plans, name):
    """Back to back, only y reset in between: no partial sum of step 1 survives into step 2 (pass 1 assigns its partial sums)."""
    c, plan = plans(name)
    x2 = integer_x(c.n, 2)
    y2 = c.reference(x2)
    assert np.any(y2 != c.y_ref)
    for x, y_ref, step in ((c.x, c.y_ref, 1), (x2, y2, 2), (c.x, c.y_ref, 3)):
        d = Dev(E, c, x).put_x(POISONS["2^60"]).put_y()
        issue(plan, d, rank_parts(c))
        assert_exact(d.y(f"{name} step {step}"), y_ref, f"{name}, step {step}")
        d.free()


# ---------------------------------------------------------------------------------------------- the stream plumbing
class Ints:
    """int32 array on the device"""

    def __init__(self, E, a):
        self.a = np.ascontiguousarray(a, dtype=np.int32)
        self.buf = E.DeviceBuffer(len(self.a) // 2 + 1)
        if len(self.a):
            assert E.host._lib.load().ehyb_h2d(self.buf.p, self.a.ctypes.data_as(C.c_void_p), self.a.nbytes) == 0

    def at(self, i=0):
        return C.c_void_p(self.buf.ptr + 4 * i)


def _vp(buf, i=0):
    return C.c_void_p(buf.ptr + 8 * i)


@pytest.mark.parametrize("n_send", [0, 1, 1023, 1024, 1025, 2500])
def test_step_pack(E, plans, n_send):
    """send_buf = x[idx] exactly, repeated indices included, nothing behind n written -- and the comm stream waits for it: a copy of
    send_buf enqueued there (what a collective does) sees the packed values."""
    lib = E.host._lib.load()
    c, _ = plans("panel-all")
    d = Dev(E, c).put_x().put_y()
    rng = np.random.default_rng(n_send)
    idx = rng.integers(0, c.n0, n_send).astype(np.int32)
    idx[::5] = idx[:1] if n_send else idx                    # one index many times
    di, ar = Ints(E, idx), Ints(E, np.arange(n_send))
    send, wire = E.DeviceBuffer(n_send + PAD).upload(np.full(n_send + PAD, SENTINEL)), E.DeviceBuffer(n_send + PAD).upload(np.full(n_send + PAD, SENTINEL))
    compute, comm = E.Stream(), E.Stream()
    assert lib.ehyb_dev_sync() == 0
    assert lib.ehyb_step_pack(_vp(d.dx), di.at() if n_send else None, _vp(send), n_send, compute.p, comm.p) == 0
    assert lib.ehyb_gather(_vp(send), ar.at(), _vp(wire), n_send, comm.p) == 0
    comm.sync(), compute.sync()
    want = np.concatenate([c.x[idx], np.full(PAD, SENTINEL)])
    assert np.array_equal(_bits(send.download()), _bits(want)), "send_buf"
    assert np.array_equal(_bits(wire.download()), _bits(want)), "the comm stream read send_buf before the pack had finished"
    d.y("pack")
    compute.destroy(), comm.destroy(), d.free()


class Wire:
    """Stands in for the collectives of a step: chunk k 'arrives' when an ehyb_gather enqueued on the comm stream copies its true
    values from a staging buffer into the ghost columns of x.  A long gather is enqueued in front of every chunk, so that a compute
    stream that does not wait for the comm stream reads the poison."""

    DELAY = 1 << 21

    def __init__(self, E, d):
        self.lib, self.d, c = E.host._lib.load(), d, d.c
        self.stage = E.DeviceBuffer(c.n).upload(d.x_true)
        self.cols = Ints(E, np.arange(c.n))
        self.delay_idx = Ints(E, np.random.default_rng(4).integers(0, c.n, self.DELAY))
        self.delay_dst = E.DeviceBuffer(self.DELAY)
        self.calls, self.fail_at = [], None

    def exchange(self, k, comm_stream, _user=None):
        self.calls.append(k)
        if k == self.fail_at:
            return 1
        _, c0, c1 = self.d.c.chunks()[k]
        rc = self.lib.ehyb_gather(_vp(self.stage), self.delay_idx.at(), _vp(self.delay_dst), self.DELAY, C.c_void_p(comm_stream))
        rc |= self.lib.ehyb_gather(_vp(self.stage), self.cols.at(c0), _vp(self.d.dx, c0), c1 - c0, C.c_void_p(comm_stream))
        self.d.hx[c0:c1] = self.d.x_true[c0:c1]
        return rc


def _send_list(E, c):
    idx = np.random.default_rng(6).integers(0, c.n0, 1500).astype(np.int32)
    return idx, Ints(E, idx), E.DeviceBuffer(len(idx) + PAD).upload(np.full(len(idx) + PAD, SENTINEL))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_a_step_through_step_part_by_hand(E, plans, name):
    """pack | own columns | chunk k on the comm stream, its part behind it on the compute stream (wait_comm) | the closing pass: x
    starts poisoned, y is exact once both streams are synchronised."""
    lib = E.host._lib.load()
    c, plan = plans(name)
    d = Dev(E, c).put_x(POISONS["nan"]).put_y()
    wire = Wire(E, d)
    idx, di, send = _send_list(E, c)
    compute, comm = E.Stream(), E.Stream()
    assert lib.ehyb_dev_sync() == 0
    assert lib.ehyb_step_pack(_vp(d.dx), di.at(), _vp(send), len(idx), compute.p, comm.p) == 0
    parts = rank_parts(c) if c.panel else [(None, 0, 1, FIRST)] + [((c0, c1), s, s + 1, LAST if s == c.n_segs - 1 else 0) for s, c0, c1 in c.chunks()]
    for k, (arrive, s0, s1, flags) in enumerate(parts):
        if arrive is not None:
            assert wire.exchange(k - 1, comm.ptr) == 0
        assert lib.ehyb_step_part(plan.h, _vp(d.dx), _vp(d.dy), compute.p, comm.p, int(arrive is not None), s0, s1, flags) == 0, lib.ehyb_last_error()
    compute.sync(), comm.sync()
    assert_exact(d.y(f"{name} by hand"), c.y_ref, f"{name}: a step through ehyb_step_part")
    assert np.array_equal(_bits(send.download()), _bits(np.concatenate([c.x[idx], np.full(PAD, SENTINEL)])))
    compute.destroy(), comm.destroy(), d.free()


@pytest.mark.parametrize("name", [n for n in PC.CASES if n != "panel-split"])   # (ehyb_halo_step never closes foreign rows)
def test_a_step_through_halo_step(E, plans, name):
    lib = E.host._lib.load()
    c, plan = plans(name)
    d = Dev(E, c).put_x(POISONS["nan"]).put_y()
    wire = Wire(E, d)
    cb = C.CFUNCTYPE(C.c_int, C.c_int, C.c_void_p, C.c_void_p)(wire.exchange)
    idx, di, send = _send_list(E, c)
    compute, comm = E.Stream(), E.Stream()
    assert lib.ehyb_dev_sync() == 0

    def step(n_chunks):
        return lib.ehyb_halo_step(plan.h, _vp(d.dx), _vp(d.dy), di.at(), _vp(send), len(idx), n_chunks, C.cast(cb, C.c_void_p), None, compute.p, comm.p)

    # a chunk count that does not match the plan's segments: refused before anything is enqueued
    plan.launched_clear()
    for bad in (c.n_segs - 2, c.n_segs, 0):
        assert step(bad) == PC.ERR_ARG
    assert wire.calls == [] and not any(plan.launched().values())
    assert np.isnan(d.y("refused")).all() and np.array_equal(_bits(send.download()), _bits(np.full(len(idx) + PAD, SENTINEL)))
    # the step
    assert step(c.n_segs - 1) == 0, lib.ehyb_last_error()
    compute.sync(), comm.sync()
    assert wire.calls == list(range(c.n_segs - 1))
    assert_exact(d.y(f"{name} halo step"), c.y_ref, f"{name}: a step through ehyb_halo_step")
    assert np.array_equal(_bits(send.download()), _bits(np.concatenate([c.x[idx], np.full(PAD, SENTINEL)])))
    # an exchange that fails aborts the step
    wire.calls, wire.fail_at = [], 1
    assert step(c.n_segs - 1) == PC.ERR_STATE and b"exchange of chunk 1 failed" in lib.ehyb_last_error()
    assert wire.calls == [0, 1]
    compute.sync(), comm.sync()
    assert lib.ehyb_dev_sync() == 0
    compute.destroy(), comm.destroy(), d.free()


# ---------------------------------------------------------------------------------------------- refusals launch nothing
def _refused(plan, d, what, code, s0, s1, flags, message):
    lib = d.lib
    plan.launched_clear()
    with pytest.raises(d.E.EhybError) as ei:
        plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, s0, s1, flags)
    assert ei.value.code == code and message in str(ei.value), (what, str(ei.value))
    assert not any(plan.launched().values()), f"{what}: the refused call had launched {plan.launched()}"
    assert lib.ehyb_dev_sync() == 0
    y = d.dy.download()
    assert np.array_equal(_bits(y), _bits(d.hy)), f"{what}: the refused call wrote y"


@pytest.mark.parametrize("name", ["panel-all", "panel-windows-kept", "csr-windows"])
def test_refusals_launch_nothing(E, plans, name):
    c, plan = plans(name)
    d = Dev(E, c).put_x().put_y(_pattern(c.n, 8))
    for flags in (LAST_FOREIGN, FIRST | LAST_FOREIGN, FIRST | LAST | LAST_FOREIGN):
        _refused(plan, d, f"{name} LAST_FOREIGN without row_split, flags {flags}", PC.ERR_STATE, 0, 1, flags, "EHYB_PART_LAST_FOREIGN needs a plan built with cfg.row_split")
    for s0, s1 in ((-1, 1), (0, c.n_segs + 1), (2, 1), (c.n_segs + 1, c.n_segs + 1)):
        _refused(plan, d, f"{name} segments [{s0}, {s1})", PC.ERR_ARG, s0, s1, FIRST | LAST, "column segments")
    # the plan still multiplies
    d.put_y()
    plan.spmv_part(d.dx.ptr, d.dy.ptr, 0, 0, c.n_segs, FIRST | LAST)
    assert_exact(d.y(name), c.y_ref, f"{name} after the refusals")
    d.free()


def test_a_plan_of_one_launch_has_no_parts(E, plans):
    c, _ = plans("csr-windows")
    m = E.Matrix.generate(*PC.CASES["csr-windows"][0][:1], *PC.CASES["csr-windows"][0][1])
    m.reorder()
    plan = E.Plan(m)                                       # defaults: the direct shape at this size
    st = plan.stats
    assert st["nnz_ell"] == 0 and st["er_segments"] == m.n and m.n == c.n0
    d = Dev(E, c).put_x().put_y(_pattern(c.n, 9))
    for flags in (FIRST | LAST, FIRST, 0):
        _refused(plan, d, f"direct shape, flags {flags}", PC.ERR_STATE, 0, 1, flags, "it has no parts")
    plan.destroy(), d.free()
