"""The *_step building blocks of the solvers (ehyb_cg_*_step, ehyb_bicgstab_*_step, ehyb_refine_*_step) on the host: every
required pointer in turn NULL, and n = -1, is EHYB_ERR_ARG with the function's own name in ehyb_last_error() -- whatever failed
before.  The checks come before the launch, so nothing here needs a GPU; no call in here gets as far as a launch."""
import ctypes as C
import re

import pytest

ERR_ARG = 1
A = 0x10000                               # never read: every call fails its argument check

# name -> (argument kinds in order: "n", "ptr" (required), "opt" (dinv: may be NULL), "int", "double", "stream")
STEPS = {
    "ehyb_cg_init_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "ptr", "stream"),
    "ehyb_cg_dot_step": ("n", "ptr", "ptr", "ptr", "stream"),
    "ehyb_cg_update_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "ptr", "int", "stream"),
    "ehyb_cg_direction_step": ("n", "ptr", "opt", "ptr", "ptr", "int", "stream"),
    "ehyb_bicgstab_init_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "ptr", "ptr", "stream"),
    "ehyb_bicgstab_dot_step": ("n", "ptr", "ptr", "ptr", "stream"),
    "ehyb_bicgstab_s_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "ptr", "int", "stream"),
    "ehyb_bicgstab_dot2_step": ("n", "ptr", "ptr", "ptr", "stream"),
    "ehyb_bicgstab_update_step": ("n", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "double", "stream"),
    "ehyb_bicgstab_direction_step": ("n", "ptr", "ptr", "opt", "ptr", "ptr", "int", "double", "stream"),
    "ehyb_refine_residual_step": ("n", "ptr", "ptr", "ptr", "ptr", "stream"),
    "ehyb_refine_axpy_step": ("n", "ptr", "ptr", "stream"),
}
GOOD = {"n": 100, "int": 0, "double": 1e-20, "stream": None}


def arguments(kinds, null=None, n=100, dinv=True):
    """null: the index of the argument passed as NULL"""
    out = []
    for i, kind in enumerate(kinds):
        if kind in ("ptr", "opt"):
            out.append(None if i == null or (kind == "opt" and not dinv) else C.c_void_p(A + 0x1000 * i))
        else:
            out.append(n if kind == "n" else GOOD[kind])
    return out


def test_the_table_is_every_step_function(E):
    """every *_step symbol of the three solver files, with the argument count the library's signature table has"""
    sigs = {k: v for k, v in E.host._lib.SIGNATURES.items() if re.fullmatch(r"ehyb_(cg|bicgstab|refine)_\w+_step", k)}
    assert set(sigs) == set(STEPS)
    for name, (_, argtypes) in sigs.items():
        assert len(argtypes) == len(STEPS[name]), name


@pytest.mark.parametrize("name", sorted(STEPS))
def test_bad_arguments_name_the_function(E, name):
    lib = E.host._lib.load()
    fn, kinds = getattr(lib, name), STEPS[name]
    other = next(k for k in sorted(STEPS) if k != name)

    def stale():                          # a different error first, so that a text left over from it would be caught
        assert getattr(lib, other)(*arguments(STEPS[other], n=-1)) == ERR_ARG
        assert other.encode() in lib.ehyb_last_error()

    required = [i for i, kind in enumerate(kinds) if kind == "ptr"]
    assert required
    for i in required:
        for dinv in (True, False):        # dinv = NULL alone is accepted: it changes nothing about which argument is at fault
            stale()
            assert fn(*arguments(kinds, null=i, dinv=dinv)) == ERR_ARG, (name, i, dinv)
            msg = lib.ehyb_last_error()
            assert name.encode() + b":" in msg and other.encode() not in msg, (name, i, msg)
    for dinv in (True, False):
        stale()
        assert fn(*arguments(kinds, n=-1, dinv=dinv)) == ERR_ARG, name
        msg = lib.ehyb_last_error()
        assert name.encode() + b":" in msg and other.encode() not in msg, (name, msg)
