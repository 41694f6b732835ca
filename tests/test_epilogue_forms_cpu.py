"""The host-side rule that picks a DMA-fed launch's compile-time epilogue form (aldm_igemm_plan_epilogue, csrc/igemm.hip
plan_epilogue_form): each form for its own combination of residual and row bias on every instantiation that carries the forms,
the generic epilogue for every disqualifier and everywhere while the process-wide switch is off.  No GPU: the planner never
dereferences a pointer."""
import ctypes

import epilogue_forms as ef
import pytest


@pytest.fixture
def L():
    from audioldm2_amd import lib
    l = lib.load()
    prev = l.aldm_igemm_epilogue_forms(1)
    yield l
    l.aldm_igemm_epilogue_forms(prev)
    l.aldm_igemm_force(0, 0, 0, 0)


def _plan(l, d, inst, splits=1):
    _fam, bm, bn, _nst, code = inst
    l.aldm_igemm_force(bm, bn, splits, 0)
    l.aldm_igemm_force_stages(code)
    try:
        form = l.aldm_igemm_plan_epilogue(ctypes.byref(d))
        assert form >= 0, l.aldm_last_error()
        stages = l.aldm_igemm_plan_stages(ctypes.byref(d))
        assert stages == code, ("the forced kernel did not take the launch", inst, stages)
        return form
    finally:
        l.aldm_igemm_force(0, 0, 0, 0)


def test_enum_and_abi():
    from audioldm2_amd import lib
    assert (lib.EPI_FORM_GENERIC, lib.EPI_FORM_PLAIN, lib.EPI_FORM_ROWBIAS, lib.EPI_FORM_RES) == (ef.GENERIC, ef.PLAIN, ef.ROWBIAS, ef.RES)
    assert lib.ABI_VERSION >= 17 and lib.load().aldm_version() == lib.ABI_VERSION
    assert lib.load().aldm_igemm_plan_epilogue(None) < 0


@pytest.mark.parametrize("inst", ef.INSTANCES, ids=ef.INSTANCE_IDS)
def test_each_form_for_its_own_combination(L, inst):
    for c in ef.cases_for(*inst[:4]):
        for split_out in (False, True):
            for bias in (True, False):
                assert _plan(L, ef.host_desc(c, bias=bias, split_out=split_out), inst) == ef.PLAIN, c["key"]
            assert _plan(L, ef.host_desc(c, res=True, split_out=split_out), inst) == ef.RES, c["key"]
            assert _plan(L, ef.host_desc(c, rowbias=True, split_out=split_out), inst) == ef.ROWBIAS, c["key"]
        # a residual AND a row bias: no form of its own
        assert _plan(L, ef.host_desc(c, res=True, rowbias=True), inst) == ef.GENERIC, c["key"]
        d = ef.host_desc(c, split_out=True)      # the split image alone (out == NULL) is an output like the other
        d.out = None
        assert _plan(L, d, inst) == ef.PLAIN, c["key"]


def _disqualified(lib, c, what):
    """-> (descriptor, split-K factor to force) of the case with one disqualifier; every one starts from a launch that gets RES."""
    d = ef.host_desc(c, res=True, split_out=what == "out_fmt")
    splits = 1
    if what == "splitk":
        d.ws, d.ws_floats = 16, 1 << 40
        splits = 2
    elif what == "geglu":
        d.epi_mode, d.res, d.ldo = lib.EPI_GEGLU, None, c["N"] // 2
    elif what == "qkv":
        d.epi_mode, d.res, d.bias, d.qkv_c, d.qkv_rows = lib.EPI_QKV, None, None, c["N"] // 3, c["M"]
        d.k_split, d.vt_split = 0x600000, 0x700000
    elif what == "act":
        d.act = lib.ACT_SILU
    elif what == "alpha":
        d.alpha = 0.5
    elif what == "accumulate":
        d.accumulate = 1
    elif what == "out_mul":
        d.out_mul, d.out_off, d.out_len = 2, 1, 2 * c["W"]
    elif what == "n_mod_4":
        d.N = d.ldo = c["N"] - 2
    elif what == "res_align":
        d.res = 0x300004
    elif what == "out_fmt":
        d.out_split_parts = 2
    else:
        raise AssertionError(what)
    return d, splits


DISQUALIFIERS = ("splitk", "geglu", "qkv", "act", "alpha", "accumulate", "out_mul", "n_mod_4", "res_align", "out_fmt")


@pytest.mark.parametrize("what", DISQUALIFIERS)
def test_every_disqualifier_forces_the_generic_form(L, what):
    from audioldm2_amd import lib
    n = 0
    for inst in ef.INSTANCES:
        fam, bm, bn, nst, _ = inst
        if fam == "halo" and what in ("geglu", "qkv", "out_mul"):
            continue                                            # (the halo kernel does not take these launches at all)
        if what == "geglu" and bn != 128:
            continue                                            # (the GEGLU epilogue needs a 128-column tile)
        if fam == "halo":
            c = ef.make_case("conv", 2, 16, 8, 64, 128, 3)
        else:   # a linear of 96 rows per sample; K = 256: eight k-tiles, the least split-K takes; N = 384: three 128-wide segments
            c = ef.make_case("linear", 1, 1, 96, 256, 384)
        base = ef.host_desc(c, res=True, split_out=what == "out_fmt")
        assert _plan(L, base, inst) == ef.RES, (inst, "the undisturbed launch must get its form")
        d, splits = _disqualified(lib, c, what)
        assert _plan(L, d, inst, splits) == ef.GENERIC, (inst, what)
        n += 1
    assert n >= 2


def test_other_kernels_and_formats_stay_generic(L):
    """Instantiations without forms: the 128x128 and 256x128 classic tiles, the 128x128 loader-wave tile and its 128x64 tile on the
    2-deep ring, the 256x128 halo tile,
    2-part images, the operand-stationary kernel, a register-staged launch."""
    c = ef.make_case("linear", 1, 1, 300, 256, 256)
    for inst in (("classic", 128, 128, 3, 3), ("classic", 256, 128, 2, 2), ("lw", 128, 128, 3, 203), ("lw", 128, 64, 2, 202),
                 ("os", 32, 128, 2, 302)):
        assert _plan(L, ef.host_desc(c, res=True), inst) == ef.GENERIC, inst
    ch = ef.make_case("conv", 2, 16, 16, 64, 128, 3)
    assert _plan(L, ef.host_desc(ch, res=True), ("halo", 256, 128, 2, 402)) == ef.GENERIC
    d = ef.host_desc(c, res=True)
    d.split_parts = 2
    assert _plan(L, d, ("classic", 64, 64, 3, 3)) == ef.GENERIC
    d = ef.host_desc(c, res=True)
    d.a_split, d.x1 = None, 0x3000
    L.aldm_igemm_force(64, 64, 1, 0)
    assert L.aldm_igemm_plan_epilogue(ctypes.byref(d)) == ef.GENERIC


def test_the_switch_forces_the_generic_form_everywhere(L):
    assert L.aldm_igemm_epilogue_forms(0) == 1
    try:
        for inst in ef.INSTANCES:
            for c in ef.cases_for(*inst[:4]):
                for kw in ({}, {"res": True}, {"rowbias": True}):
                    assert _plan(L, ef.host_desc(c, **kw), inst) == ef.GENERIC, (inst, c["key"], kw)
        assert L.aldm_igemm_epilogue_forms(0) == 0          # returns what was in force
    finally:
        assert L.aldm_igemm_epilogue_forms(1) == 0
    assert _plan(L, ef.host_desc(ef.cases_for(*ef.INSTANCES[0][:4])[0], res=True), ef.INSTANCES[0]) == ef.RES
    # any other value restores the default: on, unless $ALDM_EPI_FORMS=0
    import os
    L.aldm_igemm_epilogue_forms(-1)
    assert L.aldm_igemm_epilogue_forms(1) == (0 if os.environ.get("ALDM_EPI_FORMS") == "0" else 1)


def test_ops_wrapper():
    from audioldm2_amd import ops
    prev = ops.igemm_epilogue_forms(0)
    try:
        assert ops.igemm_epilogue_forms(1) == 0
        assert ops.igemm_epilogue_forms(prev) == 1
    finally:
        ops.igemm_epilogue_forms(prev)
