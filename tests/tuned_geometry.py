"""The shipped tuning tables as test cases (tests/test_tuned_geometries_cpu.py, tests/test_tuned_geometries_gpu.py).

A table key is ops._TUNE_FIELDS, then the prologue mode (ops._pre_mode), then "dma" / "dma2" for a launch over a pre-split A
operand.  case_from_key() turns a key into what is needed to issue exactly that launch through the public ops API;
reference_fp64() evaluates the same operation as a plain sum over taps in fp64, with torch only (any device), independent of the
library: zero padding, dilation, stride, nearest upsampling and the channel concat are index arithmetic, the prologue, GEGLU,
bias and residual are applied in fp64.  Importable without a GPU."""
import json
import math
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_DIR = os.path.join(ROOT, "audioldm2_amd", "tuning")
# (table file, which launches it serves): the four tables ops._tuned_table reads
TABLES = ("mi355x_igemm.json", "mi355x_igemm_bf16x6.json", "mi355x_igemm_dma.json", "mi355x_igemm_dma_bf16x3.json")
SHORT = {"mi355x_igemm.json": "f32", "mi355x_igemm_bf16x6.json": "bx", "mi355x_igemm_dma.json": "dma",
         "mi355x_igemm_dma_bf16x3.json": "dma2"}
# (mode to run in, A-operand format) per table: fp32 = plain tensor, "bf16" = SplitT from split_rows, "f16" = the fp16 image a
# GroupNorm / LayerNorm producer writes in "f16x3" mode
RUNS = {"mi355x_igemm.json": (("f32", "fp32"),), "mi355x_igemm_bf16x6.json": (("bf16x6", "fp32"),),
        "mi355x_igemm_dma.json": (("bf16x6", "bf16"),), "mi355x_igemm_dma_bf16x3.json": (("bf16x3", "bf16"), ("f16x3", "f16"))}
LRELU_SLOPE = 0.1
GUARD = 1 << 18          # floats of NaN on each side of an output: 1 MiB
NAN_BITS = 0x7FC00000    # torch.nan as fp32


def tune_fields():
    from audioldm2_amd import ops
    return ops._TUNE_FIELDS


def load_table(name):
    with open(os.path.join(TUNING_DIR, name)) as f:
        return json.load(f)["entries"]


def parse_key(key):
    """-> ({field: int}, pre_mode, suffix)."""
    fields = tune_fields()
    p = [s.strip() for s in key.split(",")]
    assert len(p) in (len(fields) + 1, len(fields) + 2), key
    suffix = p[len(fields) + 1] if len(p) > len(fields) + 1 else ""
    assert suffix in ("", "dma", "dma2"), key
    return {f: int(v) for f, v in zip(fields, p)}, int(p[len(fields)]), suffix


def normalise_key(key):
    f, pre, suffix = parse_key(key)
    return ",".join(str(f[n]) for n in tune_fields()) + f",{pre}" + (("," + suffix) if suffix else "")


def natural_out(size, up, pad, dil, k, stride):
    return (size * up + 2 * pad - dil * (k - 1) - 1) // stride + 1


def case_from_key(key):
    """Everything needed to issue the launch a key names through ops.linear / ops.linear_geglu / ops.conv (b_mode 0, batch 1) or
    ops.gemm_nt / ops.gemm_packed_batched (activation x activation products)."""
    f, pre, suffix = parse_key(key)
    c = {"key": normalise_key(key), "pre_mode": pre, "split": suffix or None}
    c.update({n: f[n] for n in ("B", "H", "W", "C1", "C2", "N", "KH", "KW", "OH", "OW", "batch", "pix1", "b_mode")})
    c["stride"], c["pad"], c["dil"], c["up"] = (f["SH"], f["SW"]), (f["PH"], f["PW"]), (f["DH"], f["DW"]), (f["up_h"], f["up_w"])
    c["K"] = (f["C1"] + f["C2"]) * f["KH"] * f["KW"]
    c["M"] = f["B"] * f["OH"] * f["OW"]
    c["flops"] = 2 * c["M"] * f["N"] * c["K"] * f["batch"]
    c["geglu"] = f["epi_mode"] == 1
    assert f["epi_mode"] in (0, 1), key          # EPI_QKV launches are tuned (and logged) under the plain key
    assert pre in (0, 1, 2, 3, 4), key
    one_by_one = f["KH"] == 1 and f["KW"] == 1 and f["SH"] == f["SW"] == 1 and f["PH"] == f["PW"] == 0 and f["up_h"] == f["up_w"] == 1
    if f["b_mode"] != 0 or f["batch"] != 1:
        assert one_by_one and f["B"] == f["H"] == 1 and f["C2"] == 0 and pre == 0 and not suffix and f["out_mul"] == 0, key
        c["op"] = "gemm_nt" if f["b_mode"] == 1 else "gemm_packed_batched"
        c["remap"] = c["out_hw"] = None
        return c
    if one_by_one and f["B"] == 1 and f["H"] == 1 and f["out_mul"] == 0 and f["C2"] == 0:
        c["op"] = "linear_geglu" if c["geglu"] else "linear"
    else:
        assert not c["geglu"], key
        c["op"] = "conv"
    # an explicit out_hw only where the launch asked for more output positions than the padding gives: they read zeros on the
    # right / bottom (the VAE's asymmetric-pad downsample, the polyphase ConvTranspose1d's Q = (Lout + p) // u + 2)
    nat = (natural_out(f["H"], f["up_h"], f["PH"], f["DH"], f["KH"], f["SH"]),
           natural_out(f["W"], f["up_w"], f["PW"], f["DW"], f["KW"], f["SW"]))
    c["out_hw"] = None if nat == (f["OH"], f["OW"]) else (f["OH"], f["OW"])
    c["remap"] = None
    if f["out_mul"] > 0:
        assert f["OH"] == 1, key
        c["remap"] = (f["out_mul"], f["out_mul"] - 1, f["out_mul"] * f["OW"])   # the last phase; every GEMM row is kept
    if suffix:
        assert f["C2"] == 0 and pre == 0 and f["C1"] % 32 == 0, key   # a pre-split operand takes no concat and no prologue
    return c


def derived_out_hw(c):
    """OH, OW as ops.conv derives them from the case."""
    if c["out_hw"] is not None:
        return c["out_hw"]
    return (natural_out(c["H"], c["up"][0], c["pad"][0], c["dil"][0], c["KH"], c["stride"][0]),
            natural_out(c["W"], c["up"][1], c["pad"][1], c["dil"][1], c["KW"], c["stride"][1]))


def desc_from_case(c):
    """The IgemmDesc ops would build for the case, as far as ops.tune_key reads it (pointers are placeholders: host only)."""
    from audioldm2_amd import lib
    d = lib.IgemmDesc()
    d.B, d.H, d.W, d.C1, d.C2, d.pix1 = c["B"], c["H"], c["W"], c["C1"], c["C2"], c["pix1"]
    d.up_h, d.up_w = c["up"]
    d.KH, d.KW = c["KH"], c["KW"]
    d.SH, d.SW = c["stride"]
    d.PH, d.PW = c["pad"]
    d.DH, d.DW = c["dil"]
    d.OH, d.OW = derived_out_hw(c)
    d.N, d.K, d.b_mode, d.batch = c["N"], c["K"], c["b_mode"], c["batch"]
    d.epi_mode = lib.EPI_GEGLU if c["geglu"] else lib.EPI_PLAIN
    if c["remap"]:
        d.out_mul, d.out_off, d.out_len = c["remap"]
    if c["pre_mode"] in (1, 2):
        d.pre_scale, d.pre_shift = 0x1000, 0x2000
    d.pre_act = {0: lib.ACT_NONE, 1: lib.ACT_NONE, 2: lib.ACT_SILU, 3: lib.ACT_LRELU, 4: lib.ACT_SILU}[c["pre_mode"]]
    if c["split"]:
        d.a_split, d.split_parts = 0x3000, (2 if c["split"] == "dma2" else 3)
    return d


def variant(c):
    """What makes two keys different operations rather than different sizes."""
    return (c["KH"], c["KW"], c["stride"], c["dil"], c["up"], c["remap"][0] if c["remap"] else 0, c["pre_mode"], c["C2"] > 0,
            c["geglu"])


def shrunk_key(c):
    """A key of the same variant (kernel, stride, dilation, upsampling, out_mul, prologue, concat, epilogue, and the same number of
    extra output positions past the padding) at a size a CPU evaluates in fp64 in no time."""
    B, H, W = 2, (1 if c["H"] == 1 else 6), (41 if c["H"] == 1 else 5)
    if c["op"] in ("linear", "linear_geglu"):
        B, H, W = 1, 1, 70
    C1, C2, N = 32, (32 if c["C2"] else 0), (128 if c["geglu"] else 40)
    nat_key = (natural_out(c["H"], c["up"][0], c["pad"][0], c["dil"][0], c["KH"], c["stride"][0]),
               natural_out(c["W"], c["up"][1], c["pad"][1], c["dil"][1], c["KW"], c["stride"][1]))
    OH = natural_out(H, c["up"][0], c["pad"][0], c["dil"][0], c["KH"], c["stride"][0]) + (c["OH"] - nat_key[0])
    OW = natural_out(W, c["up"][1], c["pad"][1], c["dil"][1], c["KW"], c["stride"][1]) + (c["OW"] - nat_key[1])
    v = {"B": B, "H": H, "W": W, "C1": C1, "C2": C2, "pix1": 0, "up_h": c["up"][0], "up_w": c["up"][1], "KH": c["KH"], "KW": c["KW"],
         "SH": c["stride"][0], "SW": c["stride"][1], "PH": c["pad"][0], "PW": c["pad"][1], "DH": c["dil"][0], "DW": c["dil"][1],
         "OH": OH, "OW": OW, "N": N, "b_mode": 0, "batch": 1, "epi_mode": 1 if c["geglu"] else 0,
         "out_mul": c["remap"][0] if c["remap"] else 0}
    return ",".join(str(v[n]) for n in tune_fields()) + f",{c['pre_mode']}" + (("," + c["split"]) if c["split"] else "")


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def make_inputs(c, device, seed=0):
    """Seeded inputs of a conv / linear case: activations N(0.3, 1) (a non-zero mean, so a padding or halo mistake changes the
    result), weights N(0, 1) / sqrt(K), a bias and a residual always, a prologue's scale in [0.5, 1.5] and shift N(0, 0.1)."""
    g = torch.Generator(device=device).manual_seed(1000 + seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device, dtype=torch.float32)
    C = c["C1"] + c["C2"]
    inp = {"x": rn(c["B"], c["H"], c["W"], c["C1"]) + 0.3,
           "x2": (rn(c["B"], c["H"], c["W"], c["C2"]) + 0.3) if c["C2"] else None,
           "w": rn(c["N"], C, c["KH"], c["KW"]) / math.sqrt(c["K"]), "bias": rn(c["N"]), "scale": None, "shift": None}
    OH, OW = derived_out_hw(c)
    n_out = c["N"] // 2 if c["geglu"] else c["N"]
    oshape = (c["B"], 1, c["remap"][2], n_out) if c["remap"] else (c["B"], OH, OW, n_out)
    inp["oshape"] = oshape
    inp["res"] = None if c["geglu"] else rn(*oshape)      # (the GEGLU epilogue has no residual input)
    if c["pre_mode"] in (1, 2):
        inp["scale"] = torch.rand(c["B"], C, generator=g, device=device, dtype=torch.float32) + 0.5
        inp["shift"] = rn(c["B"], C) * 0.1
    return inp


def gelu_erf(v):
    return 0.5 * v * (1.0 + torch.erf(v * (0.5 ** 0.5)))


def prologue_fp64(c, a, scale, shift):
    """pre_mode 1: a * scale + shift per (sample, channel); 2: SiLU of that; 3: LeakyReLU; 4: SiLU of the raw operand."""
    m = c["pre_mode"]
    if m in (1, 2):
        a = a * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
    if m in (2, 4):
        a = a * torch.sigmoid(a)
    if m == 3:
        a = torch.where(a > 0, a, a * LRELU_SLOPE)
    return a


def reference_fp64(c, a, w, bias=None, res=None, dtype=torch.float64):
    """(dtype = torch.float32: the same sum over the same taps with torch's fp32 matmul and fp32 accumulation — not a reference but
    the yardstick of what fp32 arithmetic itself loses on a case, logged for K >= tolerances.LONG_K; tolerances.act_act_long_k_tol.)
    a: the A operand AFTER its prologue, [B, H, W, C] (x ++ x2), any float dtype; w [N, C, KH, KW]; -> fp64 [B, OH, OW, N']
    (N' = N / 2 behind the GEGLU epilogue: rows [0, N/2) of w are the value half, the rest the gate half), + bias, + res
    (res in the layout of the launch's output: remapped rows for a polyphase case)."""
    B, H, W, C = a.shape
    OH, OW = derived_out_hw(c)
    (SH, SW), (PH, PW), (DH, DW), (UH, UW) = c["stride"], c["pad"], c["dil"], c["up"]
    dev = a.device
    a = a.to(dtype)
    acc = torch.zeros(B * OH * OW, c["N"], dtype=dtype, device=dev)
    oh, ow = torch.arange(OH, device=dev), torch.arange(OW, device=dev)
    for kh in range(c["KH"]):
        vh = oh * SH - PH + kh * DH                      # row in the (upsampled) image this tap reads
        okh = (vh >= 0) & (vh < H * UH)
        ih = vh.clamp(0, H * UH - 1) // UH               # nearest upsampling: source row
        for kw in range(c["KW"]):
            vw = ow * SW - PW + kw * DW
            okw = (vw >= 0) & (vw < W * UW)
            iw = vw.clamp(0, W * UW - 1) // UW
            t = a
            if not (OH == H and bool((ih == oh).all())):
                t = t.index_select(1, ih)
            if not (OW == W and bool((iw == ow).all())):
                t = t.index_select(2, iw)
            if not bool(okh.all()):
                t = t * okh.to(t.dtype)[None, :, None, None]
            if not bool(okw.all()):
                t = t * okw.to(t.dtype)[None, None, :, None]
            acc.addmm_(t.reshape(B * OH * OW, C), w[:, :, kh, kw].to(dtype).t())
            del t
    if bias is not None:
        acc += bias.to(dtype)
    if c["geglu"]:
        half = c["N"] // 2
        acc = acc[:, :half] * gelu_erf(acc[:, half:])
    y = acc.view(B, OH, OW, -1)
    if res is not None:
        if c["remap"]:
            mul, off, out_len = c["remap"]
            y = y + res.to(dtype).view(B, out_len, -1)[:, off::mul][:, :OW].reshape(y.shape)
        else:
            y = y + res.to(dtype).view(y.shape)
    return y


def rel_errors(y, ref):
    """(max|y - ref| / max|ref| over the whole tensor, the largest of the same ratio over each 32-column block on its own
    max|ref|, the index of that block): y, ref [..., N]."""
    N = ref.shape[-1]
    err = (y.reshape(-1, N).double() - ref.reshape(-1, N)).abs().amax(0)
    mag = ref.reshape(-1, N).abs().amax(0)
    whole = float(err.max() / mag.max())
    nb = -(-N // 32)
    pad = nb * 32 - N
    if pad:
        err = torch.cat([err, err.new_zeros(pad)])
        mag = torch.cat([mag, mag.new_zeros(pad)])
    blk = err.view(nb, 32).amax(1) / mag.view(nb, 32).amax(1)
    worst = int(blk.argmax())
    return whole, float(blk[worst]), worst


# ---- the launch ----------------------------------------------------------------------------------------------------------------
FAMILY = {0: "igemm_dma_kernel", 1: "igemm_dma_ws_kernel", 2: "igemm_dma_lw_kernel", 3: "igemm_dma_os_kernel",
          4: "igemm_dma_halo_kernel"}


def expected_dma_kernel(stages):
    """(kernel family, ring depth) a DMA table entry's stage code names: < 100 classic, 1xx persistent wave-specialised, 2xx loader
    waves, 3xx operand-stationary, 4xx halo patch (the tens digit there: 8 waves)."""
    fam = stages // 100
    return FAMILY[fam], (stages - 400) % 10 if fam == 4 else stages % 100


def ran_dma_kernel(name):
    """(family, ring depth) out of a recorded kernel name, e.g. igemm_dma_lw_kernel<128, 64, 3, 2, 3>."""
    fam, args = name.split("<")
    args = [int(s) for s in args.rstrip(">").split(",")]
    return fam, args[1] if fam == "igemm_dma_os_kernel" else args[2]


def assert_launch_is_entry(c, entry, log, prof, table):
    """Exactly one igemm launch, under the entry's key, on the entry's tile / split-K (/ wave groups / kernel family and ring depth /
    matrix-core path).  A hint the planner replaced by something else fails here."""
    assert len(log) == 1 and len(prof) == 1, (c["key"], log, [p[0] for p in prof])
    assert log[0] == c["key"], (log[0], c["key"])
    if entry is None:
        return
    what, bm, bn, _fl, _e0, _e1, shape, name = prof[0]
    splits, kgroups = shape[8] // 10, shape[8] % 10
    assert (bm, bn, splits) == tuple(entry[:3]), (c["key"], entry, (bm, bn, splits), name)
    if c["split"]:
        assert ran_dma_kernel(name) == expected_dma_kernel(entry[3]), (c["key"], entry, name)
        if entry[3] >= 400:   # the halo kernel's wave count is part of the code: 41x = 8 waves (WM = 4 on the 128-row tile too)
            wm = int(name.split("<")[1].rstrip(">").split(",")[3])
            assert wm == (4 if (bm == 256 or (entry[3] - 400) // 10) else 2), (c["key"], entry, name)
    else:
        assert max(kgroups, 1) == max(entry[3], 1), (c["key"], entry, kgroups, name)
        bx = name.rstrip(">").split(",")[-1].strip() == "true"
        if table == "mi355x_igemm.json":
            assert not bx, (c["key"], name)
        elif len(entry) > 4 and entry[4] == 1:
            assert not bx, (c["key"], entry, name, "the table sends this shape to the fp32 MFMA")
        else:
            assert bx, (c["key"], entry, name, "a bf16x6-table entry must run the bf16-split instantiation")
