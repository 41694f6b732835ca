"""What tests/test_epilogue_forms_cpu.py and tests/test_epilogue_forms_gpu.py share: the kernel instantiations that carry the
compile-time epilogue forms (csrc/igemm_epilogue.h, ALDM_EPI_FORM_*), and the small cases they are tried on, in the vocabulary of
tests/tuned_geometry.py.  Importable without a GPU."""
import tuned_geometry as tg

GENERIC, PLAIN, ROWBIAS, RES = 0, 1, 2, 3          # lib.EPI_FORM_*
FORM_NAMES = {PLAIN: "plain", ROWBIAS: "rowbias", RES: "res"}

# (family, BM, BN, ring depth, stages code of ops.igemm_force) of every instantiation with forms: the classic and loader-wave
# kernels' 64x64 / 64x128 / 128x64 tiles on 3-part images (csrc/igemm_dma_forms.hip, igemm_dma_lw_forms.hip) and the halo-patch
# kernel's 128x128 tile on 4 waves with a 4-deep and on 8 waves with a 2-deep weight ring (igemm_dma_halo_forms.hip)
# (not the loader-wave 128x64 tile on its 2-deep ring: its forms would add scratch, profiles/r10_epilogue_forms_registers.txt)
INSTANCES = [(fam, bm, bn, nst, base + nst)
             for fam, base in (("classic", 0), ("lw", 200))
             for bm, bn, rings in ((64, 64, (2, 3)), (64, 128, (2, 4)), (128, 64, (2, 4)))
             for nst in rings if (fam, bm, bn, nst) != ("lw", 128, 64, 2)] + [("halo", 128, 128, 4, 404), ("halo", 128, 128, 2, 412)]
INSTANCE_IDS = [f"{fam}-{bm}x{bn}-ring{nst}" for fam, bm, bn, nst, _ in INSTANCES]


def make_case(op, B, H, W, C1, N, k=1):
    """A case dict as tuned_geometry.case_from_key builds it: a linear over B*H*W rows (k = 1) or a k x k stride-1 'same' conv."""
    c = {"op": op, "B": B, "H": H, "W": W, "C1": C1, "C2": 0, "pix1": 0, "N": N, "KH": k, "KW": k, "stride": (1, 1),
         "pad": (k // 2, k // 2), "dil": (1, 1), "up": (1, 1), "batch": 1, "b_mode": 0, "geglu": False, "remap": None,
         "out_hw": None, "pre_mode": 0, "split": "dma", "K": C1 * k * k, "M": B * H * W}
    c["key"] = f"{op}-{B}x{H}x{W}-{C1}to{N}-k{k}"
    return c


def cases_for(fam, bm, bn, nst):
    """The smallest shapes at which a form can go wrong on this instantiation.
    classic / loader-wave: linears with M = BM + 40 rows (a partial last row tile, not a multiple of 32), N = BN + 32 (a partial
    last column tile) and N = BN, K = 64 (shorter than the ring) and K = 32 (ring + 1) (one steady k-tile); and a two-sample 3x3
    conv on a 6x5 image, 32 -> 64 channels: 60 rows, the row-bias sample changes inside the tile, OH*OW is no multiple of BM.
    halo: the kernel only runs tiles of whole image rows inside one image (W a power of two, OH*OW % BM == 0), so its smallest
    launch is a two-sample 3x3 conv on a 16x8 image (one 128-row tile per sample: the row-bias sample changes between tiles);
    64 input channels (two channel blocks: both patch buffers), N = BN + 32 and N = BN."""
    if fam == "halo":
        return [make_case("conv", 2, 16, 8, 64, n, 3) for n in (bn + 32, bn)]
    out = [make_case("linear", 1, 1, bm + 40, K, n) for n in (bn + 32, bn) for K in (64, 32 * (nst + 1))]
    out.append(make_case("conv", 2, 6, 5, 32, 64, 3))
    return out


def host_desc(c, res=False, rowbias=False, bias=True, split_out=False):
    """A descriptor of the case the host-side planner accepts (placeholder pointers: nothing is launched)."""
    d = tg.desc_from_case(c)
    d.w, d.w_split, d.out = 0x4000, 0x8000, 0x100000
    d.ldo, d.alpha = c["N"], 1.0
    if bias:
        d.bias = 0x200000
    if res:
        d.res = 0x300000
    if rowbias:
        d.rowbias = 0x400000
    if split_out:
        d.out_split, d.out_split_c = 0x500000, c["N"]
    return d
