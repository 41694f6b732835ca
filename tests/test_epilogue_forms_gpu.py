"""The compile-time epilogue forms of the DMA-fed GEMM kernels (csrc/igemm_epilogue.h: igemm_epilogue_form, ALDM_EPI_FORM_*) against
the generic run-time epilogue of the same kernels and against fp64.

Every instantiation that carries the forms (epilogue_forms.INSTANCES: kernel family, tile, ring) x every form (plain, + row bias,
+ residual), pinned with ops.igemm_force, at the shapes of epilogue_forms.cases_for, without the split-image output, with it
("also") and with it alone ("only").  For every launch:
  (a) with the forms on the fp32 output and the raw bytes of the split image are BITWISE what the same launch gives under
      ops.igemm_epilogue_forms(0) — and the launch did take the form (aldm_igemm_plan_epilogue on the descriptor ops launched), the
      generic epilogue under the switch;
  (b) the output is within tolerances.gemm_tol() of tuned_geometry.reference_fp64 (+ the row bias, added in fp64);
  (c) both outputs are views into sentinel-filled buffers with 1 MiB of guard on each side: the guards are untouched and every
      element inside was written.
And one launch per disqualifier of the host-side rule (split-K, GEGLU, QKV, an activation, alpha != 1, accumulate, a row remap,
N % 4 != 0, a misaligned residual, an output image format different from the operand's): it runs with the forms on, takes the
generic epilogue, and meets (b) — the forms did not change what the generic path computes.  The bar is gemm_tol() throughout (the
GEGLU case included: measured 4.7e-7 .. 7.7e-7 on the shipped geometries, tests/tolerances.py)."""
import contextlib
import ctypes
import math

import epilogue_forms as ef
import pytest
import torch
import tuned_geometry as tg
from tolerances import gemm_tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT16 = 0x7FC1               # int16 sentinel of the image buffers: a bf16 NaN no split ever produces (the splits truncate / round finite values)
_REF = {}                     # (case key, what) -> fp64 reference, computed once


@pytest.fixture
def ops():
    from audioldm2_amd import ops as o
    prev_mode = o.MMA_MODE
    o.set_mma("bf16x6")
    prev = o.igemm_epilogue_forms(1)
    try:
        yield o
    finally:
        o.igemm_epilogue_forms(prev)
        o.igemm_force(0, 0, 0)
        o.set_mma(prev_mode)


def _nan_buffer(numel):
    big = torch.full((numel + 2 * tg.GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    return big, big[tg.GUARD:tg.GUARD + numel]


def _guards_intact(big, numel):
    bits = big.view(torch.int32)
    return bool((bits[:tg.GUARD] == tg.NAN_BITS).all()) and bool((bits[tg.GUARD + numel:] == tg.NAN_BITS).all())


@contextlib.contextmanager
def guarded_images(ops, made):
    """While active, every split image ops allocates is a view into a sentinel-filled int16 buffer with 1 MiB of guard on each side;
    `made` collects (whole buffer, image)."""
    orig = ops.SplitT.empty
    G = 2 * tg.GUARD   # int16 elements per MiB

    def empty(shape, device, parts=None, f16_scale=0.0):
        so = orig(shape, device, parts, f16_scale)
        n = so.data.numel()
        big = torch.full((n + 2 * G,), SENT16, device=device, dtype=torch.int16)
        so.data = big[G:G + n].view(so.data.shape)
        made.append((big, so))
        return so
    ops.SplitT.empty = staticmethod(empty)
    try:
        yield
    finally:
        ops.SplitT.empty = staticmethod(orig)


def _image_guards_intact(big, so):
    G, n = 2 * tg.GUARD, so.data.numel()
    return bool((big[:G] == SENT16).all()) and bool((big[G + n:] == SENT16).all())


@contextlib.contextmanager
def recorded_forms(ops, forms):
    """While active, `forms` collects the epilogue form of every igemm launch ops issues: aldm_igemm_plan_epilogue on the very
    descriptor, after the launch (ops has filled in its hints and workspace by then), under the same force and switch settings."""
    from audioldm2_amd import lib
    orig = ops._igemm

    def igemm(d, what, *a, **k):
        orig(d, what, *a, **k)
        forms.append(lib.load().aldm_igemm_plan_epilogue(ctypes.byref(d)))
    ops._igemm = igemm
    try:
        yield
    finally:
        ops._igemm = orig


def _inputs(c):
    inp = tg.make_inputs(c, DEV, seed=7)
    g = torch.Generator(device=DEV).manual_seed(4242)
    inp["rowbias"] = torch.randn(c["B"], c["N"], generator=g, device=DEV, dtype=torch.float32)
    return inp


def _contraction(c, inp):
    """fp64 sum over taps alone (no bias, no residual), [B, OH, OW, N]; computed once per case."""
    k = (c["key"], "acc")
    if k not in _REF:
        _REF[k] = tg.reference_fp64(c, inp["x"], inp["w"])
    return _REF[k]


def _epilogue64(acc, bias=None, rowbias=None, act=None, res=None, alpha=1.0, prev=None):
    """v = act(acc + bias + rowbias); v = alpha (v + res); out = prev + v — in fp64."""
    v = acc.clone()
    if bias is not None:
        v += bias.double()
    if rowbias is not None:
        v += rowbias.double()[:, None, None, :]
    if act == "silu":
        v = v * torch.sigmoid(v)
    if res is not None:
        v += res.double().view(v.shape)
    v *= alpha
    if prev is not None:
        v += prev.double().view(v.shape)
    return v


def _rel(y, ref):
    return float((y.double().reshape(ref.shape) - ref).abs().max() / ref.abs().max())


def _launch(ops, c, xs, pw, inp, form, split_out, big_out, out):
    """One launch of the case in the given form; -> (fp32 view or None, SplitT or None, [(buffer, image)], [forms])."""
    kw = {"split_out": split_out}
    if form == ef.RES:
        kw["res"] = inp["res"]
    if form == ef.ROWBIAS:
        kw["rowbias"] = inp["rowbias"]
    if split_out != "only":
        big_out.fill_(float("nan"))
        kw["out"] = out
    made, forms = [], []
    with guarded_images(ops, made), recorded_forms(ops, forms):
        if c["op"] == "linear":
            r = ops.linear(xs.view(1, c["W"], c["C1"]), pw, **kw)
        else:
            r = ops.conv(xs, pw, stride=c["stride"], pad=c["pad"], **kw)
    torch.cuda.synchronize()
    y, so = (None, r) if split_out == "only" else (r if split_out else (r, None))
    return y, so, made, forms


@pytest.mark.parametrize("form", (ef.PLAIN, ef.ROWBIAS, ef.RES), ids=lambda f: ef.FORM_NAMES[f])
@pytest.mark.parametrize("inst", ef.INSTANCES, ids=ef.INSTANCE_IDS)
def test_form_is_bitwise_the_generic_epilogue_and_matches_fp64(ops, inst, form):
    fam, bm, bn, nst, code = inst
    bar = gemm_tol()
    for c in ef.cases_for(fam, bm, bn, nst):
        inp = _inputs(c)
        xs = ops.split_rows(inp["x"])
        assert xs.fmt == "bf16" and xs.parts == 3
        pw = ops.pack_conv(inp["w"][:, :, 0, 0] if c["op"] == "linear" else inp["w"], inp["bias"])
        ref = _epilogue64(_contraction(c, inp), inp["bias"], inp["rowbias"] if form == ef.ROWBIAS else None,
                          res=inp["res"] if form == ef.RES else None)
        numel = math.prod(inp["oshape"])
        big, out = _nan_buffer(numel)
        ops.igemm_force(bm, bn, 1, 0, code)
        try:
            for split_out in (None, "also", "only"):
                tag = (inst, ef.FORM_NAMES[form], c["key"], split_out)
                got = {}
                for on in (1, 0):
                    prev = ops.igemm_epilogue_forms(on)
                    try:
                        y, so, made, forms = _launch(ops, c, xs, pw, inp, form, split_out, big, out)
                    finally:
                        ops.igemm_epilogue_forms(prev)
                    assert forms == [form if on else ef.GENERIC], (tag, on, forms)
                    # (c) nothing outside the outputs, everything inside written
                    if y is not None:
                        assert _guards_intact(big, numel), (tag, on, "the launch wrote outside its fp32 output")
                        assert not bool(torch.isnan(y).any()), (tag, on, "an fp32 output element was never written")
                    assert len(made) == (1 if split_out else 0), (tag, len(made))
                    for bigi, img in made:
                        assert _image_guards_intact(bigi, img), (tag, on, "the launch wrote outside its split image")
                        assert not bool((img.data == SENT16).any()), (tag, on, "a split-image element was never written")
                    # (b) against fp64: the fp32 output, and the image (an exact 3-part split of the same values)
                    if y is not None:
                        e = _rel(y, ref)
                        print(f"{tag} forms={on} fp32 out: {e:.3e} (bar {bar:.1e})")
                        assert e < bar, (tag, on, e, bar)
                    if so is not None:
                        e = _rel(so.float(), ref)
                        print(f"{tag} forms={on} image:    {e:.3e} (bar {bar:.1e})")
                        assert e < bar, (tag, on, "image", e, bar)
                        if y is not None:
                            assert torch.equal(so.float().view(-1), y.reshape(-1)), (tag, on, "the 3-part image is the exact split of out")
                    got[on] = (None if y is None else y.clone(), None if so is None else so.data.clone())
                # (a) bitwise the generic epilogue
                if got[1][0] is not None:
                    assert torch.equal(got[1][0].view(torch.int32), got[0][0].view(torch.int32)), (tag, "fp32 output differs")
                if got[1][1] is not None:
                    assert torch.equal(got[1][1], got[0][1]), (tag, "split image differs")
        finally:
            ops.igemm_force(0, 0, 0)


# ---- (d) one launch per disqualifier: generic epilogue with the forms on, right against fp64 -------------------------------------
def _run_generic(ops, force, fn):
    forms = []
    ops.igemm_force(*force)
    try:
        with recorded_forms(ops, forms):
            r = fn()
        torch.cuda.synchronize()
    finally:
        ops.igemm_force(0, 0, 0)
    assert forms == [ef.GENERIC], forms
    return r


DISQUALIFIERS = ("splitk", "geglu", "qkv", "act", "alpha", "accumulate", "out_mul", "n_mod_4", "res_align", "out_fmt")


@pytest.mark.parametrize("what", DISQUALIFIERS)
def test_disqualified_launch_takes_the_generic_epilogue_and_matches_fp64(ops, what):
    from audioldm2_amd import lib
    bar = gemm_tol()
    M, K = (96 if what == "qkv" else 104), 256         # 64 + 40 rows (QKV: whole 32-key tiles); eight k-tiles: the least split-K takes
    force = (64, 64, 1, 0, 3)                          # classic 64x64, ring 3: an instantiation WITH forms
    N = {"geglu": 128, "qkv": 192, "n_mod_4": 66}.get(what, 96)
    c = ef.make_case("linear", 1, 1, M, K, N)
    c["key"] += "-" + what
    if what == "geglu":
        c["geglu"], force = True, (64, 128, 1, 0, 2)   # (the GEGLU epilogue needs the 128-column tile)
    inp = _inputs(c)
    x, w, bias, res = inp["x"], inp["w"], inp["bias"], inp["res"]
    xs = ops.split_rows(x)
    x3 = xs.view(1, M, K)
    # the undisturbed launch gets the residual form: what follows is generic because of the disqualifier alone
    if what not in ("geglu", "qkv", "n_mod_4", "out_fmt"):
        forms = []
        ops.igemm_force(*force)
        try:
            with recorded_forms(ops, forms):
                ops.linear(x3, ops.pack_conv(w[:, :, 0, 0], bias), res=res)
        finally:
            ops.igemm_force(0, 0, 0)
        assert forms == [ef.RES], forms
    if what == "geglu":
        pw = ops.pack_geglu(w[:, :, 0, 0], bias)
        y = _run_generic(ops, force, lambda: ops.linear_geglu(x3, pw))
        ref = tg.reference_fp64(c, x, w, bias)
    elif what == "qkv":
        pw = ops.pack_conv(w[:, :, 0, 0], None)
        q, k_img, _vt = _run_generic(ops, force, lambda: ops.linear_qkv(x3, pw, heads=2, rows_per_sample=M))
        ref = _contraction(c, inp)
        kf = (k_img.to(torch.int32) << 16).view(torch.float32).sum(2).reshape(M, 64)     # [M, heads, parts, 32] -> the k columns
        e = _rel(kf, ref[..., 64:128])
        print(f"qkv k image: {e:.3e} (bar {bar:.1e})")
        assert e < bar, ("qkv k", e, bar)
        y, ref = q, ref[..., :64]
    elif what == "out_fmt":
        # "f16x3": the operand is a 2-part fp16 image from a LayerNorm, the output image 3-part bf16
        ops.set_mma("f16x3")
        g = torch.Generator(device=DEV).manual_seed(99)
        gamma = torch.rand(K, generator=g, device=DEV) + 0.5
        beta = torch.randn(K, generator=g, device=DEV) * 0.1
        xs16 = ops.layernorm(x.view(1, M, K), gamma, beta, 1e-5, split_out="only")
        assert xs16.fmt == "f16" and xs16.parts == 2
        pw = ops.pack_conv(w[:, :, 0, 0], bias)
        y, so = _run_generic(ops, force, lambda: ops.linear(xs16, pw, res=res, split_out="also"))
        assert so.fmt == "bf16" and so.parts == 3
        a = xs16.float().view(1, 1, M, K)      # the image's own values (hi + lo, exact in fp32): the reference multiplies those
        ref = _epilogue64(tg.reference_fp64(c, a, w), bias, res=res)
        assert torch.equal(so.float().view(-1), y.reshape(-1))
    else:
        pw = ops.pack_conv(w[:, :, 0, 0], bias)
        acc = _contraction(c, inp)
        if what == "splitk":
            y = _run_generic(ops, (64, 64, 2, 0, 3), lambda: ops.linear(x3, pw, res=res))
            ref = _epilogue64(acc, bias, res=res)
        elif what == "act":
            y = _run_generic(ops, force, lambda: ops.linear(x3, pw, res=res, act=ops.ACT_SILU))
            ref = _epilogue64(acc, bias, act="silu", res=res)
        elif what == "alpha":
            y = _run_generic(ops, force, lambda: ops.linear(x3, pw, res=res, alpha=0.5))
            ref = _epilogue64(acc, bias, res=res, alpha=0.5)
        elif what == "accumulate":
            prev = torch.randn(1, M, N, device=DEV)
            out = prev.clone()
            y = _run_generic(ops, force, lambda: ops.linear(x3, pw, res=res, out=out, accumulate=True))
            ref = _epilogue64(acc, bias, res=res, prev=prev)
        elif what == "out_mul":
            # rows (0, q) land at 2 q + 1 of a [1, 1, 2 M, N] output; the residual is read there too
            out = torch.full((1, 1, 2 * M, N), float("nan"), device=DEV)
            res2 = torch.randn(1, 1, 2 * M, N, device=DEV)
            r = _run_generic(ops, force, lambda: ops.conv(xs.view(1, 1, M, K), pw, res=res2, out=out, remap=(2, 1, 2 * M)))
            assert bool(torch.isnan(r[0, 0, 0::2]).all()), "rows of the other phase must stay untouched"
            y = r[0, 0, 1::2]
            ref = _epilogue64(acc, bias, res=res2[0, 0, 1::2].reshape(1, 1, M, N))
        elif what == "n_mod_4":
            y = _run_generic(ops, force, lambda: ops.linear(x3, pw, res=res))
            ref = _epilogue64(acc, bias, res=res)
        elif what == "res_align":
            buf = torch.empty(M * N + 4, device=DEV)
            res1 = buf[1:1 + M * N].view(1, 1, M, N)
            res1.copy_(res)
            assert res1.data_ptr() % 16 == 4
            y = _run_generic(ops, force, lambda: ops.linear(x3, pw, res=res1))
            ref = _epilogue64(acc, bias, res=res)
        else:
            raise AssertionError(what)
    assert not bool(torch.isnan(y).any())
    e = _rel(y, ref)
    print(f"{what}: generic epilogue with the forms on, {e:.3e} (bar {bar:.1e})")
    assert e < bar, (what, e, bar)
    assert lib.load().aldm_igemm_epilogue_forms(1) == 1      # the switch was on throughout
