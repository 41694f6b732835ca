"""Every geometry of the four shipped tuning tables, launched through the public ops API at its real size, on the kernel its
entry names, against fp64.

Which igemm kernel a launch runs is a table lookup (audioldm2_amd/tuning/mi355x_igemm*.json: 578 entries, the geometries of the
benchmark and of the shipped model configs).  For each entry (the bf16x3 DMA table twice: 2-part bf16 images in "bf16x3", fp16
images from a GroupNorm / LayerNorm producer in "f16x3" — 751 launches):

  * the launch is the entry: one igemm launch is logged, under the entry's key, and what ops.PROFILE records of it — tile, split-K,
    wave groups / kernel family and ring depth, matrix-core path — is what the entry says.  A hint the planner silently replaced
    fails here;
  * output hygiene: the output is a view into a NaN-filled buffer with 1 MiB of guard on each side; the guards (and, for a
    polyphase remap, the rows of the other phases) are bit-for-bit NaN afterwards, the output holds none, a second launch is
    bitwise equal;
  * the result against tuned_geometry.reference_fp64 (a sum over taps of fp64 matmuls, evaluated with torch on the GPU: the
    largest cases are 2.5 TFLOP), max|y - ref| / max|ref| under gemm_tol(mode) — fused_tol(mode) behind a prologue, in front of the
    GEGLU, or in "f16x3", where the reference normalises in fp64 — over the whole tensor AND over every 32-column block on the
    block's own max|ref|.

WHAT THIS FILE FOUND (measured on an MI355X).  With one fp32 accumulator over the whole K loop, 23 entries — 2 of the bf16x6
table, 21 of the DMA table, all "bf16x6", plain epilogue, K = 3072 .. 11520 at split-K 1 — sat at 2.0e-6 .. 3.0e-6 whole / up to
3.4e-6 on their worst 32-column block, above gemm_tol's 2e-6, where torch's fp32 matmul over the same taps loses 2.6e-7 .. 8.0e-7:
no bar of its own was due to the class.  The K loops of the DMA-fed classic, halo and loader-wave kernels and of the 128x128
register-staged tiles without an affine prologue now accumulate in blocks of K = 1024 (acc_close_block, csrc/igemm_epilogue.h).
On that library every case of this file passes (profiles/r08_tuned_geometry_errors.txt): the plain K >= 3072 split-K 1 entries
measure 3.9e-7 .. 7.3e-7 whole / 4.7e-7 .. 7.6e-7 worst block in the DMA table (42 entries) and 4.3e-7 .. 5.3e-7 / 5.0e-7 ..
6.7e-7 in the bf16x6 table (3), next to torch fp32's 2.6e-7 .. 8.0e-7 / 3.0e-7 .. 9.8e-7.  The bars are the existing ones.

The fused q | k | v projections are tuned under the plain key of their geometry: those keys also run ops.linear_qkv.  And one test
per mode logs every launch of the benchmark's UNet pass, VAE decode and vocoder pass and puts whatever the tables do not hold
through the same check."""
import math

import pytest
import torch
import tuned_geometry as tg
from tolerances import LONG_K, act_act_long_k_tol, fp32_grade, fused_tol, gemm_tol, log_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cases():
    out, ids = [], []
    for name in tg.TABLES:
        entries = tg.load_table(name)
        for mode, fmt in tg.RUNS[name]:
            for i, (key, v) in enumerate(entries.items()):
                c = tg.case_from_key(key)
                out.append((name, key, mode, fmt))
                tag = tg.SHORT[name] + ("-f16" if fmt == "f16" else "")
                ids.append(f"{tag}-{i:03d}-{c['M']}x{c['N']}x{c['K']}")
    return out, ids


CASES, IDS = _cases()
assert len(CASES) == 145 + 97 + 163 + 2 * 173


def _qkv_cases():
    """DMA 1x1 keys of the form ops.linear_qkv launches (B = H = 1: it flattens the rows) with N = 3 C1."""
    out, ids = [], []
    for name in tg.TABLES[2:]:
        for mode, fmt in tg.RUNS[name]:
            for i, key in enumerate(tg.load_table(name)):
                c = tg.case_from_key(key)
                if c["op"] == "linear" and c["N"] == 3 * c["C1"]:
                    out.append((name, key, mode, fmt))
                    ids.append(f"{tg.SHORT[name]}{'-f16' if fmt == 'f16' else ''}-{i:03d}-qkv-{c['M']}x{c['N']}x{c['K']}")
    return out, ids


QKV_CASES, QKV_IDS = _qkv_cases()


@pytest.fixture
def ops():
    from audioldm2_amd import ops as o
    prev = o.MMA_MODE
    yield o
    o.set_mma(prev)
    o.TUNE_LOG = None
    o.PROFILE = None


def _nan_buffer(numel):
    big = torch.full((numel + 2 * tg.GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    return big, big[tg.GUARD:tg.GUARD + numel]


def _guards_intact(big, numel):
    bits = big.view(torch.int32)
    return bool((bits[:tg.GUARD] == tg.NAN_BITS).all()) and bool((bits[tg.GUARD + numel:] == tg.NAN_BITS).all())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _group_norm_fp64(x, gamma, beta, silu, groups=32, eps=1e-5):
    B, H, W, C = x.shape
    v = x.double().view(B, H * W, groups, C // groups)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((v - mean) / torch.sqrt(var + eps)).view(B, H, W, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def _layer_norm_fp64(x, gamma, beta, eps=1e-5):
    v = x.double()
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def _operand(ops, c, fmt, inp, seed):
    """-> (what the launch takes as x, the fp64-able A operand after its prologue [B, H, W, C])."""
    x = inp["x"]
    if fmt == "fp32":
        a = x if inp["x2"] is None else torch.cat([x, inp["x2"]], -1)
        return x, tg.prologue_fp64(c, a.double(), inp["scale"], inp["shift"])
    if fmt == "bf16":                       # the exact 3-part image in "bf16x6", (hi, mid) rounded to nearest in "bf16x3":
        xs = ops.split_rows(x)              # the reference keeps the fp32 values either way
        assert xs.fmt == "bf16" and xs.parts == (2 if c["split"] == "dma2" else 3), (xs.fmt, xs.parts)
        return xs, x
    assert fmt == "f16" and ops.f16_mode()
    g = _gen(5000 + seed)
    C = c["C1"]
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV) * 0.1
    if c["op"] in ("linear", "linear_geglu") and C <= 2048:   # a LayerNorm feeds the projections: the image carries the rows' norm
        xs = ops.layernorm(x.view(1, c["W"], C), gamma, beta, 1e-5, split_out="only")     # bound (the kernel's rows end at 2048)
        a = _layer_norm_fp64(x, gamma, beta)
    else:                                        # GroupNorm (+ SiLU in front of a convolution) feeds everything else
        silu = c["op"] == "conv"
        xs = ops.gn_split(x, gamma, beta, groups=32, eps=1e-5, act=ops.ACT_SILU if silu else ops.ACT_NONE)
        a = _group_norm_fp64(x, gamma, beta, silu)
    assert xs.fmt == "f16" and xs.parts == 2
    return xs, a


def check_key(ops, key, mode, fmt, entry=None, table=None, seed=0, bar_mode=None):
    """The per-key check of the module docstring; entry = None: whatever the cost model plans (only the key is asserted)."""
    c = tg.case_from_key(key)
    assert ops.MMA_MODE == mode
    inp = tg.make_inputs(c, DEV, seed)
    xop, a = _operand(ops, c, fmt, inp, seed)
    w, bias, res = inp["w"], inp["bias"], inp["res"]
    pw = ops.pack_geglu(w[:, :, 0, 0], bias) if c["geglu"] else ops.pack_conv(w[:, :, 0, 0] if c["op"] == "linear" else w, bias)
    kw = {}
    if c["pre_mode"] in (1, 2):
        kw["pre"] = (inp["scale"], inp["shift"])
    if c["pre_mode"] in (2, 4):
        kw["pre_act"] = ops.ACT_SILU
    if c["pre_mode"] == 3:
        kw["pre_act"], kw["pre_slope"] = ops.ACT_LRELU, tg.LRELU_SLOPE
    oshape = inp["oshape"]
    numel = math.prod(oshape)
    big, out = _nan_buffer(numel)

    def launch():
        if c["op"] == "linear_geglu":
            return ops.linear_geglu(xop.view(1, c["W"], c["C1"]), pw, out=out)
        if c["op"] == "linear":
            return ops.linear(xop.view(1, c["W"], c["C1"]), pw, res=res, out=out, **kw)
        return ops.conv(xop, pw, stride=c["stride"], pad=c["pad"], dil=c["dil"], up=c["up"], x2=inp["x2"], out_hw=c["out_hw"],
                        res=res, out=out, remap=c["remap"], **kw)

    ops.TUNE_LOG, ops.PROFILE = [], []
    try:
        launch()
        torch.cuda.synchronize()
        log, prof = ops.TUNE_LOG, ops.PROFILE
    finally:
        ops.TUNE_LOG = ops.PROFILE = None
    tg.assert_launch_is_entry(c, entry, log, prof, table)

    assert _guards_intact(big, numel), "the launch wrote outside its output"
    N = oshape[-1]
    if c["remap"]:
        mul, off, out_len = c["remap"]
        rows = out.view(c["B"], out_len, N)
        y = rows[:, off::mul][:, :c["OW"]]
        assert int((rows.view(torch.int32) == tg.NAN_BITS).sum()) == c["B"] * (out_len - c["OW"]) * N, \
            "rows of the other phases must stay untouched"
    else:
        y = out.view(oshape)
    assert not bool(torch.isnan(y).any()), "an output element was never written"
    first = out.clone()
    big.fill_(float("nan"))
    launch()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32)), "a second identical launch must be bitwise equal"
    assert _guards_intact(big, numel)
    del first

    ref = tg.reference_fp64(c, a, w, bias, res)
    whole, blk, worst = tg.rel_errors(y, ref)
    fused = c["pre_mode"] != 0 or c["geglu"] or fmt == "f16"
    bar = (fused_tol if fused else gemm_tol)(bar_mode or mode)
    if not fused and c["K"] >= LONG_K and fp32_grade(bar_mode or mode):
        # what torch's fp32 matmul loses on the very same taps, logged next to the kernel's figure (the bar stays gemm_tol)
        y32 = tg.reference_fp64(c, a, w, bias, res, dtype=torch.float32)
        w32, b32, _ = tg.rel_errors(y32, ref)
        del y32
        print(f"{key} torch fp32 matmul over the same taps: whole {w32:.3e} worst 32-column block {b32:.3e}")
        log_err(w32, 0.0, "torch-fp32.whole")
        log_err(b32, 0.0, "torch-fp32.block32")
    del a
    print(f"{key} [{mode}/{fmt}] whole {whole:.3e} worst 32-column block {blk:.3e} (block {worst}) bar {bar:.1e}")
    log_err(whole, bar, "whole")
    log_err(blk, bar, "block32")
    del ref, y, out, big
    if numel > (1 << 27):
        torch.cuda.empty_cache()
    assert whole < bar, (key, whole, bar)
    assert blk < bar, (key, "32-column block", worst, blk, bar)


@pytest.mark.parametrize("table,key,mode,fmt", CASES, ids=IDS)
def test_table_entry_runs_its_kernel_and_matches_fp64(ops, table, key, mode, fmt):
    ops.set_mma(mode)
    check_key(ops, key, mode, fmt, entry=tg.load_table(table)[key], table=table, seed=CASES.index((table, key, mode, fmt)) % 997)


# ---- the fused q | k | v projection -----------------------------------------------------------------------------------------------
def _unet_attention_rows():
    """{channel width: (heads, rows per sample)} of the self-attentions of the benchmark's UNet (oracle/cases.py UNET_FULL on the
    256 x 16 latent of a 10.24 s clip): level i runs at (256 >> i) x (16 >> i) tokens with model_channels * channel_mult[i]."""
    from oracle import cases
    cfg = cases.UNET_FULL
    out = {}
    for i, m in enumerate(cfg["channel_mult"]):
        if (1 << i) in cfg["attention_resolutions"]:
            C = cfg["model_channels"] * m
            out[C] = (C // cfg["num_head_channels"], (256 >> i) * (16 >> i))
    return out


def _image_to_fp64(img, part_dim, scale):
    if scale:   # fp16 parts of scale * value
        return img.view(torch.float16).double().sum(part_dim) / scale
    return (img.to(torch.int32) << 16).view(torch.float32).double().sum(part_dim)


@pytest.mark.parametrize("table,key,mode,fmt", QKV_CASES, ids=QKV_IDS)
def test_qkv_form_of_a_table_entry(ops, table, key, mode, fmt):
    """ops.linear_qkv on the tabled geometry (EPI_QKV launches are tuned under the plain key): the launch is the entry, q and the K /
    V^T images against the fp64 projection (V^T per 32-key tile as a multiset — the tile's key order is the attention kernel's
    own — and through the attention over the images against fp64 attention, which also pins the order), bitwise repeatable."""
    ops.set_mma(mode)
    c = tg.case_from_key(key)
    entry = tg.load_table(table)[key]
    C, M = c["C1"], c["W"]
    heads, L = _unet_attention_rows()[C]
    assert M % L == 0 and heads * 32 == C
    B = M // L
    g = _gen(77)
    x = torch.randn(B, L, C, generator=g, device=DEV) + 0.3
    w = torch.randn(3 * C, C, generator=g, device=DEV) / math.sqrt(C)
    pw = ops.pack_conv(w)
    if fmt == "f16":
        gamma = torch.rand(C, generator=g, device=DEV) + 0.5
        beta = torch.randn(C, generator=g, device=DEV) * 0.1
        xs = ops.layernorm(x, gamma, beta, 1e-5, split_out="only")
        a = _layer_norm_fp64(x, gamma, beta)
        assert xs.fmt == "f16" and xs.rn > 0.0
    else:
        xs, a = ops.split_rows(x), x.double()
        assert xs.parts == (2 if c["split"] == "dma2" else 3)
    ops.TUNE_LOG, ops.PROFILE = [], []
    try:
        q, k_img, vt_img = ops.linear_qkv(xs, pw, heads, L)
        torch.cuda.synchronize()
        log, prof = ops.TUNE_LOG, ops.PROFILE
    finally:
        ops.TUNE_LOG = ops.PROFILE = None
    tg.assert_launch_is_entry(c, entry, log, prof, table)
    q2, k2, v2 = ops.linear_qkv(xs, pw, heads, L)
    assert torch.equal(q, q2) and torch.equal(k_img, k2) and torch.equal(vt_img, v2), "a second identical launch must be bitwise equal"
    f16s = getattr(k_img, "_aldm_f16", None)
    assert (f16s is not None) == (fmt == "f16")
    ref = a.view(M, C) @ w.double().t()
    qr, kr, vr = ref[:, :C], ref[:, C:2 * C], ref[:, 2 * C:]
    bar = (fused_tol if fmt == "f16" else gemm_tol)(mode)
    kd = _image_to_fp64(k_img, 2, f16s[1] if f16s else 0.0).reshape(M, C)
    for name, got, want in (("q", q.view(M, C), qr), ("k", kd, kr)):
        whole, blk, worst = tg.rel_errors(got, want)
        print(f"{key} [{mode}/{fmt}] {name}: whole {whole:.3e} worst head {blk:.3e} bar {bar:.1e}")
        log_err(whole, bar, name + ".whole")
        log_err(blk, bar, name + ".block32")
        assert whole < bar and blk < bar, (name, whole, blk, worst, bar)
    # V^T: [b][head][tile][part][32 dims][32 keys]
    vd = _image_to_fp64(vt_img, 3, f16s[2] if f16s else 0.0)                                    # [B, heads, L/32, 32 d, 32 keys]
    vw = vr.reshape(B, L // 32, 32, heads, 32).permute(0, 3, 1, 4, 2)                          # the same axes from the reference
    err = (vd.sort(-1).values - vw.sort(-1).values).abs().amax((0, 2, 4))                       # per (head, dim)
    mag = vw.abs().amax((0, 2, 4))
    whole, blk = float(err.max() / mag.max()), float((err.amax(1) / mag.amax(1)).max())
    print(f"{key} [{mode}/{fmt}] v^T: whole {whole:.3e} worst head {blk:.3e} bar {bar:.1e}")
    log_err(whole, bar, "vt.whole")
    log_err(blk, bar, "vt.block32")
    assert whole < bar and blk < bar, ("v^T", whole, blk, bar)
    att = ops.attention_presplit(q, k_img, vt_img, heads)
    sh = lambda t: t.reshape(B, L, heads, 32).transpose(1, 2)
    p = torch.softmax(sh(qr) @ sh(kr).transpose(-1, -2) * 32 ** -0.5, -1)
    want = (p @ sh(vr)).transpose(1, 2).reshape(M, C)
    del p
    whole, blk, worst = tg.rel_errors(att.view(M, C), want)
    print(f"{key} [{mode}/{fmt}] attention over the images: whole {whole:.3e} worst head {blk:.3e} bar {fused_tol(mode):.1e}")
    log_err(whole, fused_tol(mode), "attn.whole")
    assert whole < fused_tol(mode), (whole, fused_tol(mode))


# ---- the headline job launches nothing the sweep did not see ---------------------------------------------------------------------------
MODE_TABLES = {"bf16x6": ("mi355x_igemm_bf16x6.json", "mi355x_igemm_dma.json"),
               "bf16x3": ("mi355x_igemm_bf16x6.json", "mi355x_igemm_dma_bf16x3.json"),
               "f16x3": ("mi355x_igemm_bf16x6.json", "mi355x_igemm_dma.json", "mi355x_igemm_dma_bf16x3.json")}


@pytest.fixture(scope="module")
def headline():
    """The benchmark's model as bench.py builds it: audioldm2-full, random-init under seed 1234, batch 8 (x 2 for guidance)."""
    from audioldm2_amd.pipeline import build_model, make_batch_for_text_to_audio
    torch.manual_seed(1234)
    ld = build_model(model_name="audioldm2-full").to(torch.device("cuda", torch.cuda.current_device()))
    if torch.is_tensor(ld.scale_factor):
        ld.scale_factor.fill_(0.75)
    ld.latent_t_size = 256
    return ld, make_batch_for_text_to_audio("synthetic prompt", batchsize=8)


def _check_batched_key(ops, key):
    """An activation x activation product (ops.gemm_nt / ops.gemm_packed_batched: the VAE mid attention) rebuilt from its key."""
    c = tg.case_from_key(key)
    Z, M, K, N = c["batch"], c["W"], c["C1"], c["N"]
    g = _gen(31)
    big, out = _nan_buffer(Z * M * N)
    out = out.view(Z, M, N)
    if c["op"] == "gemm_nt":
        lda = c["pix1"] or K
        a = (torch.randn(Z, M, lda, generator=g, device=DEV) + 0.3)[:, :, :K]
        b = torch.randn(Z, N, K, generator=g, device=DEV) / math.sqrt(K)
        launch = lambda: ops.gemm_nt(a, b, out=out)
        ref = a.double() @ b.double().transpose(1, 2)
    else:
        a = torch.randn(Z, M, K, generator=g, device=DEV) + 0.3
        b = torch.randn(Z, K, N, generator=g, device=DEV) / math.sqrt(K)
        bp = ops.pack_kn(b)
        launch = lambda: ops.gemm_packed_batched(a, bp, K, N, out=out)
        ref = a.double() @ b.double()
    ops.TUNE_LOG, ops.PROFILE = [], []
    try:
        launch()
        torch.cuda.synchronize()
        log, prof = ops.TUNE_LOG, ops.PROFILE
    finally:
        ops.TUNE_LOG = ops.PROFILE = None
    tg.assert_launch_is_entry(c, None, log, prof, None)
    assert _guards_intact(big, Z * M * N) and not bool(torch.isnan(out).any())
    first = out.clone()
    launch()
    assert torch.equal(first, out)
    whole, blk, worst = tg.rel_errors(out, ref)
    bar = gemm_tol("f32")     # no split image of an activation can exist: these run the fp32 MFMA in every mode
    if K >= LONG_K:
        y32 = (a.float() @ b.float().transpose(1, 2)) if c["op"] == "gemm_nt" else (a.float() @ b.float())
        w32, b32, _ = tg.rel_errors(y32, ref)
        del y32
        print(f"{key} torch fp32 matmul: whole {w32:.3e} worst 32-column block {b32:.3e}")
        log_err(w32, 0.0, "torch-fp32.whole")
        log_err(b32, 0.0, "torch-fp32.block32")
        bar = act_act_long_k_tol()
    print(f"{key} [{c['op']}] whole {whole:.3e} worst 32-column block {blk:.3e} bar {bar:.1e}")
    log_err(whole, bar, "whole")
    log_err(blk, bar, "block32")
    assert whole < bar and blk < bar, (key, whole, blk, worst, bar)


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3", "f16x3"])
def test_headline_job_launches_nothing_the_sweep_did_not_see(ops, headline, mode):
    """One eager UNet pass at the benchmark's shape (batch 8 x guidance), one VAE decode and one vocoder pass at batch 8 with every
    launch's key logged: a weight GEMM's key is in one of the mode's tables (then the sweep above ran exactly that launch) or goes
    through the same per-key check on whatever the cost model plans; activation x activation products likewise through
    ops.gemm_nt / ops.gemm_packed_batched.  A key that cannot be rebuilt fails the test.  Table entries this job never launches
    (other models' geometries, other batch sizes) are counted, not failed."""
    ld, batch = headline
    ops.set_mma(mode)
    B = 8
    with torch.no_grad():
        cond = ld.get_learned_conditioning_dict(batch)
        uncond = {k: ld.cond_stage_models[m["model_idx"]].get_unconditional_condition(B)
                  for k, m in ld.cond_stage_model_metadata.items()}
        x = torch.randn(B, ld.channels, ld.latent_t_size, ld.latent_f_size, device=DEV)
        z = torch.randn(B, ld.channels, ld.latent_t_size, ld.latent_f_size, device=DEV)
        t2 = torch.full((2 * B,), 501.0, device=DEV)
        ops.TUNE_LOG = []
        try:
            ld.apply_model_cfg(x, t2, cond, uncond)
            mel = ld.decode_first_stage_cl(z)
            ld.first_stage_model.vocoder.forward_cl(mel.view(mel.shape[0], mel.shape[1], mel.shape[2]).float().contiguous())
            torch.cuda.synchronize()
            logged = ops.TUNE_LOG
        finally:
            ops.TUNE_LOG = None
    del mel, x, z
    keys = sorted(set(logged))
    assert len(logged) > 100 and len(keys) > 30, (len(logged), len(keys))
    tabled = {k for name in MODE_TABLES[mode] for k in tg.load_table(name)}
    n_tabled, untabled, failures = 0, [], []
    for key in keys:
        c = tg.case_from_key(key)            # (asserts on a key it cannot parse)
        if key in tabled:
            n_tabled += 1
            continue
        untabled.append(key)
        # Every key is judged, so one missed bar does not hide the next.  Only a failed assertion is collected: any other error
        # (a HIP error reaches Python as a RuntimeError) ends the test at once, and nothing more is launched after it.
        try:
            if c["op"] in ("gemm_nt", "gemm_packed_batched"):
                _check_batched_key(ops, key)
            else:
                # a register-staged launch runs the six-product kernels in every mode (ops.py, MMA_MODE): the fp32-grade bars
                fmt = "fp32" if c["split"] is None else ("f16" if (c["split"] == "dma2" and mode == "f16x3") else "bf16")
                check_key(ops, key, mode, fmt, entry=None, seed=len(untabled), bar_mode=None if c["split"] else "bf16x6")
        except AssertionError as e:
            failures.append((key, repr(e)[:400]))
    # NOT "stale": the tables also hold the other three models' geometries and other batch sizes, which this one job never launches
    not_in_this_job = sorted(tabled - set(keys))
    print(f"[{mode}] {len(logged)} launches, {len(keys)} distinct keys: {n_tabled} tabled, {len(untabled)} untabled (checked here), "
          f"{len(not_in_this_job)} of the {len(tabled)} entries of this mode's tables not launched by this one job (audioldm2-full)")
    for key in untabled:
        print(f"  untabled: {key}")
    assert not failures, failures
