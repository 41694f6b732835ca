/*
 * aldm_hip.h — C ABI of libaldm_hip.so, the MI355X (gfx950) kernel library behind the
 * AudioLDM2 sampling hot path (DDIM/UNet -> VAE decode -> HiFi-GAN, + STFT/mel).
 *
 * The reference (haoheliu/AudioLDM2) has NO native code: every "kernel" on this path is an
 * ATen op reached from Python.  The entry points below are therefore the op inventory of
 * SURVEY.md §2.3, one C function per fused op; each comment cites the reference call site
 * (file:line under /root/reference/audioldm2/) whose arithmetic the entry point replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensors), fp32,
 *     channels-last ("tokens x C": [B, H, W, C] / [B, L, C]); no torch types cross this ABI;
 *   - `stream` is a hipStream_t passed as void*; nothing here synchronises or allocates;
 *   - return value: 0 on success, negative on error; aldm_last_error() gives the message
 *     (thread local).  Host wrappers turn that into a Python RuntimeError, mirroring the
 *     reference's plain-exception convention (e.g. openaimodel.py:858-860 asserts).
 *   - operands, accumulators and every stored tensor are IEEE fp32; HOW an fp32 x fp32 product of a contraction is
 *     evaluated depends on the matrix-core mode: "f32" = v_mfma_f32_32x32x2_f32 (exact fp32 products,
 *     bit-identical to an fmaf chain); "bf16x6" (the DEFAULT) = 6 bf16 MFMA partial products of exact 3-part operand
 *     splits (fp32 grade, 2.4e-7 rms vs fp64); "bf16x3" (opt-in fast mode for launches over pre-split operands and for
 *     attention) = 3 partial products of (hi, mid) parts rounded to nearest: 16 significant bits per operand, 4.4e-6 rms.
 */
#ifndef ALDM_HIP_H
#define ALDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library / error ------------------------------------------------------------------ */
int aldm_version(void);              /* ABI version (27),bumped on any struct / entry change */
const char* aldm_last_error(void);   /* message of the last failing call on this thread     */

/* ---- activations usable as prologue (applied to the gathered input) or epilogue -------- */
enum {
    ALDM_ACT_NONE = 0,
    ALDM_ACT_SILU = 1,      /* x*sigmoid(x): util.py:219-221, model.py:33-35                */
    ALDM_ACT_LRELU = 2,     /* leaky_relu(x, slope): hifigan/models.py:98,151,161           */
    ALDM_ACT_TANH = 3,      /* hifigan/models.py:163                                        */
    ALDM_ACT_LOGCLAMP = 4,  /* log(max(x, slope)): audio_processing.py:85-91 (clip 1e-5)    */
    ALDM_ACT_GELU = 5,      /* exact erf GELU: attention.py:44                              */
    ALDM_ACT_GELU_TANH = 6  /* tanh GELU ("gelu_new"): GPT-2 MLP of the sequence generator, sequence_input.py:69 */
};

/* epilogue modes of aldm_igemm.
 * ALDM_EPI_GEGLU: the GEMM computes the 2*C-wide GEGLU projection, but only C columns are
 * stored: out[m, g*32 + l] = (acc[m, g*64 + l] + bias) * gelu_erf(acc[m, g*64 + 32 + l] + bias),
 * i.e. the weight's output channels are interleaved in groups of 32 (value block, gate block)
 * — pack with aldm_pack_weight from a weight whose rows were permuted that way.  N (the packed
 * width, 2*C) must be a multiple of 64, ldo >= N/2, no split-K, rowbias unused; act = ALDM_ACT_GELU_TANH selects the tanh
 * GELU for the gate (the gated-GELU FF of the FLAN-T5 conditioner: wo(gelu_new(wi_0 x) * wi_1 x)), otherwise erf GELU. */
/* ALDM_EPI_QKV (ABI v6, DMA-fed launches only): the fused self-attention projection [q | k | v] = x W^T (N = 3*qkv_c, no
 * bias; attention.py:335-342) whose epilogue hands the attention kernel its operands in the form it multiplies them in:
 *   columns [0, C)    q   -> out, fp32 [M, ldo >= C]
 *   columns [C, 2C)   k   -> k_split: the split image [M][C/32][parts][32] of the k columns (a head = one 32-channel block)
 *   columns [2C, 3C)  v   -> vt_split: v TRANSPOSED per (sample, head, 32-key tile), written straight from the MFMA accumulator
 *                            layout (no LDS transposition): [b][head][tile][part][32 dims][32 keys] bf16, the keys of a tile in
 *                            the order the attention kernel's P^T operand holds them (chunk 2s + lh = accumulator registers 8s ..
 *                            8s + 7 of lane half lh, i.e. tile rows (r & 3) + 8 (r >> 2) + 4 lh).
 * Requires C % 32 == 0, the block tile's width dividing C, qkv_rows (rows per sample) % 32 == 0 dividing M, no split-K.  ABI v10:
 * qkv_rows may also be M rounded up to 32 — one padded sample, the form a token count L % 32 != 0 takes (a 32-row slab would
 * straddle two samples): aldm_vt_regroup then turns that v^T image into the per-sample one of ceil(L / 32) tiles.  The split is the
 * one aldm_attention_d32 applies to fp32 K / V in registers (split_parts = 2: (hi, mid) round to nearest; 3: exact), so
 * aldm_attention_d32_presplit over these images gives bit-identical results with ~30 % fewer VALU instructions per key tile. */
enum { ALDM_EPI_PLAIN = 0, ALDM_EPI_GEGLU = 1, ALDM_EPI_QKV = 2 };

/* B-operand layouts of aldm_igemm */
enum {
    ALDM_B_PACKED = 0, /* weights pre-packed by aldm_pack_weight: [ceil(K/4)][Npad][4]      */
    ALDM_B_NT = 1      /* row-major activations Bmat[N][ldb] (C = A * Bmat^T)               */
};

/*
 * aldm_igemm — the one contraction engine: implicit-GEMM convolution on fp32 MFMA.
 *   out[m, n] = epi( sum_k A[m, k] * W[k, n] ),  m = (b, oh, ow),  k = (kh, kw, ci)
 * A is gathered on the fly from one or two channels-last tensors (x1 ++ x2 along C = the
 * UNet skip concat, openaimodel.py:879), optionally through a virtual nearest-neighbour
 * upsample (openaimodel.py:133, model.py:54), optionally through a per-(sample, channel)
 * affine + activation (= GroupNorm apply + SiLU fused into the conv: openaimodel.py:227-231,
 * model.py:156-158; or leaky_relu for HiFi-GAN).  Zero padding stays zero.
 * Replaces: nn.Conv2d (openaimodel.py:122,172,230,256,267,572,810; attention.py:439,452;
 * model.py:49,139,147,195-203,596,650; autoencoder.py:112), nn.Conv1d / ConvTranspose1d
 * (hifigan/models.py:24-84,114-141), nn.Linear (attention.py:40,54,335-342;
 * openaimodel.py:244-250,537-541), F.conv1d DFT basis (stft.py:67-72), torch.bmm
 * (model.py:219,226), torch.matmul mel basis (stft.py:174).
 */
enum { ALDM_MMA_F32 = 0, ALDM_MMA_BF16X6 = 1 };

typedef struct aldm_igemm_desc {
    /* A operand: gathered input */
    const float* x1;       /* [B, H, W, C1] channels-last                                   */
    const float* x2;       /* optional second tensor, concatenated after x1 along C         */
    int32_t C1, C2;        /* channels of x1 / x2 (C2 = 0 when x2 == NULL); multiples of 4  */
    int32_t pix1, pix2;    /* element pitch between consecutive pixels (0 => C1 / C2)       */
    int32_t B, H, W;       /* stored input extent                                           */
    int32_t up_h, up_w;    /* virtual nearest upsample factors (1 = none)                   */
    int32_t KH, KW, SH, SW, PH, PW, DH, DW;
    int32_t OH, OW;        /* output extent; M = B*OH*OW                                    */
    /* prologue on A */
    const float* pre_scale; /* [B, C1+C2] or NULL: a = a*scale + shift                      */
    const float* pre_shift;
    int32_t pre_act;        /* ALDM_ACT_* applied after the affine                          */
    float pre_slope;
    /* B operand */
    const float* w;
    int32_t b_mode;        /* ALDM_B_PACKED / ALDM_B_NT                                     */
    int32_t ldb;           /* NT: row pitch of Bmat; PACKED: Npad                           */
    int32_t K, N;          /* K = KH*KW*(C1+C2) (multiple of 4), N = output channels        */
    /* epilogue: v = act(acc + bias[n] + rowbias[b, n]); v = alpha*(v + res[m, n]);
       out = accumulate ? out + v : v   (HiFi-GAN: xs += (resblock_j(x))/num_kernels)        */
    const float* bias;     /* [N] or NULL                                                   */
    const float* rowbias;  /* [B, rowbias_ld] or NULL (timestep-embedding add, openaimodel.py:298) */
    const float* res;      /* [Mout, ldo] or NULL (residual)                                */
    float* out;            /* [Mout, ldo]                                                   */
    int32_t ldo;           /* output row pitch in elements (>= N)                           */
    int32_t act;           /* ALDM_ACT_* epilogue                                           */
    float act_slope;
    float alpha;
    int32_t accumulate;
    /* output row remap (polyphase ConvTranspose1d, hifigan/models.py:127-134): when
       out_mul > 0 the GEMM row (b, q) is stored at row b*out_len + q*out_mul + out_off and
       dropped when that position falls outside [0, out_len).  Requires OH == 1.            */
    int32_t out_mul, out_off, out_len;
    /* batched GEMM: blockIdx.z = batch; element strides added per batch (0 = shared)       */
    int32_t batch;
    int64_t stride_x, stride_w, stride_o;
    /* ABI v2 */
    int32_t rowbias_ld;    /* row pitch of rowbias (0 => N): lets every ResBlock read its slice of
                              ONE batched timestep-embedding projection                          */
    int32_t epi_mode;      /* ALDM_EPI_*: 0 = plain; ALDM_EPI_GEGLU fuses attention.py:42-44 (GEGLU)
                              into the projection GEMM — see below                               */
    float* ws;             /* optional split-K workspace (caller-owned scratch, see
                              aldm_igemm_ws_floats); NULL or too small => no split-K            */
    int64_t ws_floats;     /* capacity of ws in floats                                          */
    /* ABI v3: tuned launch configuration for this shape (0 = pick with the built-in cost model):
       block tile hint_bm x hint_bn in {128x128,128x64,64x128,64x64,128x32} and split-K factor.
       audioldm2_amd/tuning/ (JSON) holds the table measured on MI355X (tools/igemm_autotune.py).  */
    int32_t hint_bm, hint_bn, hint_splits;
    int32_t hint_kgroups;  /* 2 = two 4-wave groups per block share the 64x64 tile's K loop (in-block
                              split-K through LDS: no workspace, no reduce kernel); 0/1 = one group */
    /* ABI v4: optional bf16-split image of the packed weights (aldm_pack_split_bf16).  When set (packed
       weights, stride_w == 0) the product runs on the bf16 matrix cores as fp32 = 6 bf16 partial products
       of exact 3-way operand splits with fp32 accumulation ("BF16x6": per-product error 0.7 * 2^-24 on average, <= 2^-21 worst case, i.e. fp32
       grade) instead of the fp32 MFMA.  NULL => fp32 MFMA.                         */
    const void* w_split;
    int32_t hint_mma;      /* tuned table: 1 = fp32 MFMA even when w_split is set, 0 = automatic          */
    int32_t hint_stages;   /* DMA-fed kernel: LDS ring depth (0 = automatic); 100 + depth = the persistent wave-
                              specialised form (one 512-thread block per CU walks a run of tiles: 4 waves run the K
                              loops, 4 waves the previous tile's epilogue) when the launch qualifies: no split-K /
                              activation / row remap / accumulate, whole tiles, 16-byte aligned operands            */
    /* ABI v5: pre-split operands ("split images", see aldm_split_rows).  When a_split is set the A operand is NOT
       gathered from x1/x2 but from the split image of the [B, H, W, C1] input (C1 % 32 == 0, C2 = 0, no prologue:
       normalisation / activation were applied by whoever wrote the image) and both operands go global -> LDS by
       DMA (global_load_lds) with no staging registers and no operand arithmetic in the K loop; requires w_split.
       out_split: the epilogue also (out != NULL) or only (out == NULL) writes its result as a split image with
       out_split_c channels per row — the A operand of the next GEMM (N % 4 == 0, 16-byte aligned out / res).    */
    const void* a_split;
    void* out_split;
    int32_t out_split_c;
    int32_t split_parts;   /* parts of a_split, of out_split and of the w_split the DMA-fed kernel reads: 3 (or 0) =
                              exact 3-way split, 6 partial products ("bf16x6"); 2 = (hi, mid) rounded to nearest, 3
                              partial products ("bf16x3": ~16 significant bits per operand, unbiased).  The register-
                              staged kernels always use the 3-part w_split.                                      */
    /* ABI v6: an activation applied to the SPLIT-IMAGE output only (ALDM_ACT_NONE | ALDM_ACT_LRELU with out_split_slope):
       out = v (fp32, e.g. a HiFi-GAN ResBlock's running sum x + conv(...), hifigan/models.py:96-103) while out_split =
       split(leaky_relu(v)), the pre-activated operand of the next conv — the leaky_relu that the register-staged kernels
       apply in their operand gather.                                                                            */
    int32_t out_split_act;
    float out_split_slope;
    /* ABI v6: ALDM_EPI_QKV outputs (see the enum) */
    void* k_split;
    void* vt_split;
    int32_t qkv_c;         /* C = heads * 32                                                                         */
    int32_t qkv_rows;      /* rows (keys) per sample                                                                  */
    /* ABI v9: "f16x3" operands.  a_fmt = ALDM_FMT_F16: a_split and w_split are 2-part images (split_parts = 2) whose parts are
       IEEE fp16 — hi = RN_f16(s x), lo = RN_f16(s x - hi), s an exact power of two chosen by the producer so that |s x| <= 65504
       holds by construction (GroupNorm / LayerNorm outputs: sqrt(n) max|gamma| + max|beta|; weights: their maximum) — and the fp32
       product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 / 16x16x32_f16: three matrix instructions instead of bf16x6's
       six, 22 of 24 significand bits per operand (measured 0.65 - 0.7x the fp32 MFMA's error against fp64:
       profiles/r06_f16x3_accuracy.txt).  acc_scale = 1 / (s_a s_w) multiplies the accumulators before the epilogue (0 = 1).
       out_split_parts: parts of the split images the EPILOGUE writes (out_split, k_split, vt_split), always bf16; 0 = split_parts.
       DMA-fed launches only (aldm_split_rows_act / aldm_groupnorm_split / aldm_layernorm_split with f16_scale != 0 write such
       images, aldm_pack_split_f16 the weights').                                                                      */
    int32_t a_fmt;
    float acc_scale;
    int32_t out_split_parts;
    /* out_split_fmt = ALDM_FMT_F16: out_split (plain and GEGLU epilogues; not k_split / vt_split) is written as the 2-part fp16
       image of out_split_scale * result — the A operand of a following f16x3 launch.  The caller vouches for |out_split_scale *
       result| <= 65504 (e.g. the GEGLU output of a LayerNorm-fed projection: (R c + b)^2 with R the row 2-norm bound of the
       normalised rows, c the largest column 2-norm of the weight, b the largest |bias|).                                  */
    int32_t out_split_fmt;
    float out_split_scale;
    /* ALDM_EPI_QKV with out_split_fmt = ALDM_FMT_F16: k_split is the fp16 image of out_split_scale * k, vt_split of vt_scale * v
       (aldm_attention_d32_presplit_f16 reads them)                                                                       */
    float vt_scale;
} aldm_igemm_desc;

int aldm_igemm(const aldm_igemm_desc* d, void* stream);
/* Floats of split-K workspace this descriptor would use (0 = the launch fills the chip without
 * splitting K).  Deep UNet levels have M = B*H*W of only 1024..4096 rows: their K loop is split
 * over blockIdx.y, partial tiles go to ws and a second kernel reduces them in a fixed order and
 * applies the epilogue (deterministic, no atomics).                                            */
int64_t aldm_igemm_ws_floats(const aldm_igemm_desc* d);
/* Host-only query (no launch): the block tile / split-K factor aldm_igemm would pick for this
 * descriptor and the algorithmic FLOPs of the call (2*M*N*K*batch) — used by bench.py's roofline
 * accounting.  splits / kgroups may be NULL.                                                              */
enum { ALDM_FMT_BF16 = 0, ALDM_FMT_F16 = 1 };
int aldm_igemm_plan(const aldm_igemm_desc* d, int* bm, int* bn, int64_t* flops, int* splits, int* kgroups,
                    int* mma);   /* mma: ALDM_MMA_* the launch would run on (may be NULL) */
/* Host-only query: LDS ring depth of the DMA-fed kernel this descriptor launches (a_split set), 0 for the register-
 * staged kernels, negative on an invalid descriptor.                                                            */
int aldm_igemm_plan_stages(const aldm_igemm_desc* d);
/* ABI v17: compile-time epilogue forms of the DMA-fed kernels (csrc/igemm_epilogue.h).  A launch with the plain epilogue, no
 * split-K, no activation, alpha == 1, no accumulate, no row remap, N % 4 == 0 and 16-byte aligned / float4-pitched out, res, bias
 * and rowbias, whose split-image output (if any) has the operand's bf16 format, on a kernel instantiation that has the forms (the
 * classic and loader-wave kernels' 64x64 / 64x128 / 128x64 tiles and the halo-patch kernel's 128x128 tile, 3-part bf16 images),
 * runs a straight-line epilogue whose bias / residual / row-bias quads are fetched before the K loop: PLAIN (bias or nothing),
 * ROWBIAS, RES.  A launch with both a residual and a row bias, and every other launch, runs the GENERIC run-time epilogue.
 * Results are bit for bit the same either way.                                                                              */
enum { ALDM_EPI_FORM_GENERIC = 0, ALDM_EPI_FORM_PLAIN = 1, ALDM_EPI_FORM_ROWBIAS = 2, ALDM_EPI_FORM_RES = 3 };
/* Host-only query: the ALDM_EPI_FORM_* aldm_igemm would run this descriptor's epilogue in (under the current force / switch
 * settings), negative on an invalid descriptor.                                                                          */
int aldm_igemm_plan_epilogue(const aldm_igemm_desc* d);
/* Process-wide switch (tests / A-B runs): on = 0 sends every launch to the generic epilogue, on = 1 enables the forms, any other
 * value restores the default (on, or $ALDM_EPI_FORMS=0: off).  Returns the value that was in force (0 / 1).                  */
int aldm_igemm_epilogue_forms(int on);
/* Tuning override (tests / tools): force the block tile and split-K factor of subsequent
 * aldm_igemm calls on this thread; bm = 0 => automatic.  bm x bn in {128x128,128x64,64x128,64x64,128x32}. */
void aldm_igemm_force(int bm, int bn, int splits, int kgroups);
/* ... and the LDS ring depth of the DMA-fed kernel (a_split descriptors): 128x128 {2,3}, 64x128 / 128x64 {2,4},
 * 64x64 {2,3}; 0 = default for the tile; 100 + depth = the persistent wave-specialised kernel (64x128 {3,4,5}, 128x64
 * {3,4}, 64x64 {4,6} on 2-part images; 64x128 / 128x64 {2,3}, 64x64 {3,4} on 3-part images); 200 + depth = the loader-wave
 * form; 300 + depth = the OPERAND-STATIONARY kernel for short K (csrc/igemm_dma_os.h: 1x1 / linear launches with K = 256 or
 * 384, the weight slab of a 128-column block held in registers, A streamed in 32-row stages of the whole K; depth 2-3 on
 * 3-part images (K = 384: 2), 2-4 on 2-part ones; 300 = the deepest ring that fits; forced with bm = 32, bn = 128) — a forced
 * launch one of them cannot run fails, a hinted one falls back to aldm_igemm's own choice.  aldm_igemm_force() resets it to 0. */
void aldm_igemm_force_stages(int stages);
/* Tuning override (tests / tools): bit mask of the block tiles that run with 8 instead of 4 wavefronts per
 * tile on this thread (1: 128x128, 2: 64x128, 4: 128x64 — GroupNorm-prologue launches; 8: 128x128 launches
 * without a prologue too).  mask < 0 restores the default (1, or $ALDM_IGEMM_W8).  Returns the mask in force. */
int aldm_igemm_wave8_mask(int mask);
/* Matrix-core path override (tests / tools) for this thread: 0 = automatic (bf16-split when the descriptor
 * carries w_split and the tuned hint allows), 1 = fp32 MFMA always, 2 = bf16-split wherever an instantiation
 * exists.  Returns the previous mode; other values only query.                                            */
int aldm_igemm_mma(int mode);
#ifdef ALDM_TEST_HOOKS
/* TEST HOOK — NOT in libaldm_hip.so (ABI v9).  It exists only in the variant library libaldm_hip_testhooks.so, which the build
 * compiles from the same sources with -DALDM_TEST_HOOKS and which tests/test_dma_gpu.py loads in a subprocess through
 * $ALDM_LIB_PATH.  Process wide: on != 0 makes DMA-fed launches leave out the smallest of the six bf16 partial products (hi_a x
 * lo_w) — a deliberately broken "5-product" GEMM, ~1e-5 off — so that the test can show that the fp32-grade tolerance WOULD catch
 * a kernel that silently lost a product.  Only the classic 64x128 tile with 2 stages and 3-part images has
 * that instantiation: while the switch is on every other aldm_igemm launch FAILS (nothing runs at full precision by accident).
 * Returns the previous setting.                                                                                          */
int aldm_debug_drop_product(int on);
#endif
/* bf16-split image of a packed weight [ceil(K/4)][Npad][4] (aldm_pack_weight / aldm_pack_kn output) for
 * aldm_igemm_desc.w_split: [4*ceil(K/32) k-octets][3 parts][Npad][8 bf16], w = hi + mid + lo exactly.
 * aldm_split_bytes = size of that image.                                                                 */
int64_t aldm_split_bytes(int K, int N);
int aldm_pack_split_bf16(const float* packed, void* dst, int K, int N, void* stream);
/* the same with `parts` = 2 | 3 parts per weight ([k-octet][parts][Npad][8 bf16]; 2 = (hi, mid) rounded to nearest,
 * the "bf16x3" image of the DMA-fed kernel)                                                                     */
int64_t aldm_split_bytes_parts(int K, int N, int parts);
int aldm_pack_split_bf16_parts(const float* packed, void* dst, int K, int N, int parts, void* stream);
/* the "f16x3" weight image (ABI v9): [k-octet][2 parts][Npad][8 fp16] of scale * w, scale an exact power of two with
 * |scale * w| <= 65504 (the caller's: 2^floor(log2(32768 / max|w|))); same size as the 2-part bf16 image (aldm_split_bytes_parts(K, N, 2)) */
int aldm_pack_split_f16(const float* packed, void* dst, int K, int N, float scale, void* stream);

/* ---- split images: pre-split activations for the DMA-fed GEMM (aldm_igemm_desc.a_split, ABI v5) -----------------
 * A split image of channels-last fp32 rows [rows, C] (C % 32 == 0) holds every value as its exact 3-way truncation
 * split x = hi + mid + lo (bf16 bit patterns), blocked [row][C/32][part][32]: 6 bytes per element, 192 contiguous
 * bytes per (row, 32-channel block); with parts = 2 ("bf16x3") only (hi, mid), both rounded to nearest: 4 bytes per
 * element, 128 bytes per block.  Producers: aldm_split_rows (below), aldm_layernorm_split,
 * aldm_attention_d32_split and aldm_igemm's out_split.                                                            */
int64_t aldm_split_image_bytes(int64_t rows, int C, int parts);
/* dst = split(act(x*scale[b, c] + shift[b, c])) with x = x1 ++ x2 along C ([rows, C1] / [rows, C2], P rows per
 * sample; scale/shift [rows/P, C1+C2] or NULL = no affine; act = ALDM_ACT_NONE | ALDM_ACT_SILU): GroupNorm apply +
 * SiLU (openaimodel.py:227-231,280-283; attention.py:459) and the skip concat (openaimodel.py:879) done ONCE per
 * element instead of once per conv tap inside the GEMM.  dst_raw (optional): split(x) of the same rows (the 1x1 skip
 * conv's operand, openaimodel.py:267).                                                                            */
int aldm_split_rows(const float* x1, const float* x2, int C1, int C2, int64_t rows, int P, const float* scale,
                    const float* shift, int act, void* dst, void* dst_raw, int parts, void* stream);
/* the same with act = ALDM_ACT_LRELU(slope) allowed as well (ABI v6): the leaky_relu in front of every HiFi-GAN conv
 * (hifigan/models.py:98, 151) applied once while writing the operand image                                          */
int aldm_split_rows_act(const float* x1, const float* x2, int C1, int C2, int64_t rows, int P, const float* scale,
                        const float* shift, int act, float slope, void* dst, void* dst_raw, int parts, void* stream);
/* "f16x3" producers (ABI v9; aldm_igemm_desc.a_fmt): dst is the 2-part IEEE-fp16 image of f16_scale * value — hi = RN_f16, lo =
 * RN_f16 of the remainder, 128 bytes per (row, 32-channel block) like a 2-part bf16 image — where f16_scale is an exact power of two
 * under which the CALLER guarantees |f16_scale * value| <= 65504 (a GroupNorm output cannot exceed sqrt(elements per group) *
 * max|gamma| + max|beta|, a LayerNorm output sqrt(C) * max|gamma| + max|beta|, SiLU only shrinks; values beyond are clamped).
 * dst_raw stays a bf16 image with raw_parts parts: raw activations have no a-priori bound.                                  */
int aldm_split_rows_f16(const float* x1, const float* x2, int C1, int C2, int64_t rows, int P, const float* scale,
                        const float* shift, int act, float slope, void* dst, void* dst_raw, int raw_parts, float f16_scale,
                        void* stream);

/* Pack a weight for ALDM_B_PACKED.  src is the PyTorch layout:
 *   conv:      [N, Cin, KH, KW] (Conv2d / Conv1d with KH = 1),  linear: KH = KW = 1
 *   transposed=1: ConvTranspose1d layout [Cin, N, KW]; phase/stride select the polyphase
 *   taps kw = phase + j*stride (j = 0..T-1, T = ceil(KWfull/stride)), stored flipped so the
 *   phase runs as an ordinary conv with PW = T-1 (polyphase decomposition, ops.pack_convtr1d).
 * dst has ceil(K/4) * Npad * 4 floats, Npad = round_up(N, 32), K = KH*KWeff*Cin.           */
int aldm_pack_weight(const float* src, float* dst, int N, int Cin, int KH, int KW,
                     int transposed, int phase, int stride, void* stream);
/* [K, N] row-major activations -> packed [ceil(K/4)][Npad][4] (P*V of the VAE attention)   */
int aldm_pack_kn(const float* src, float* dst, int K, int N, int lds, int batch,
                 int64_t stride_src, int64_t stride_dst, void* stream);

/* ---- normalisation -------------------------------------------------------------------- */
/* GroupNorm statistics over channels-last x = x1 ++ x2 -> per-(b, c) scale/shift such that
 * GroupNorm(x)[b, p, c] = x*scale[b, c] + shift[b, c]  (scale = rstd*gamma,
 * shift = beta - mean*rstd*gamma).  util.py:224-241 (eps 1e-5), attention.py:75-78 and
 * model.py:38-41 (eps 1e-6).  ws: scratch of aldm_gn_ws_floats() floats.
 * Statistics are accumulated about a per-thread pivot and merged with the parallel-variance formula in fp64 (fixed
 * order), so |mean| >> std inputs keep their variance (ATen: Welford). */
int aldm_groupnorm_stats(const float* x1, const float* x2, int B, int P, int C1, int C2,
                         int G, float eps, const float* gamma, const float* beta,
                         float* scale, float* shift, float* ws, void* stream);
int64_t aldm_gn_ws_floats(int B, int P, int C, int G);
/* The launch form of a GroupNorm (ABI v15; host only, no launch), from the one function the launchers follow: want_split = 0 asks
 * for aldm_groupnorm_stats, 1 for aldm_groupnorm_split{,_f16}.  form: ALDM_GN_CHUNKED = partial statistics per (pixel chunk,
 * sample) + a finalize launch (+ aldm_split_rows for a split); ALDM_GN_FUSED = one launch whose blocks own whole groups (+
 * aldm_split_rows for a split); ALDM_GN_FUSED_SPLIT = statistics, apply, activation and operand split in that one launch.
 * group_slices x groups_per_block = G is the rule's block ownership (the fused grid is (group_slices, B); more than 4 groups per
 * block, B >= 64 with G = 32, sends even a small sample to the chunked form, whose blocks each see all G groups); chunks x chunk_px
 * the chunked grid (1 x P when fused); cols x rows the 256-thread block as float4 columns x pixel rows; passes the column passes
 * of a block; active_threads the threads of a block's first pass that hold data.  $ALDM_GN_FUSED_MAX and $ALDM_GN_SPLIT_FUSED
 * (read once) act inside.  Out pointers may be NULL.  For tests, which reach a form by shape and assert here which one.        */
enum { ALDM_GN_CHUNKED = 0, ALDM_GN_FUSED = 1, ALDM_GN_FUSED_SPLIT = 2 };
int aldm_groupnorm_plan(int B, int P, int C1, int C2, int G, int want_split, int* form, int* group_slices,
                        int* groups_per_block, int* chunks, int* chunk_px, int* cols, int* rows, int* passes,
                        int* active_threads);
/* GroupNorm + activation (ALDM_ACT_NONE | ALDM_ACT_SILU) + operand split in one call (ABI v6): dst = split(act(GroupNorm(x1 ++
 * x2))) as a split image with `parts` parts, dst_raw (optional) = split(x1 ++ x2) — the image aldm_groupnorm_stats followed by
 * aldm_split_rows writes, bit for bit.  Samples of up to 1024 pixels run as ONE launch (a block owns whole groups: it reads its
 * channel slab for the statistics, then normalises and splits it while it is still in L2); larger ones as the two launches.
 * scale / shift [B, C1+C2] are written as by aldm_groupnorm_stats.                                                       */
int aldm_groupnorm_split(const float* x1, const float* x2, int B, int P, int C1, int C2, int G, float eps,
                         const float* gamma, const float* beta, int act, float* scale, float* shift, float* ws,
                         void* dst, void* dst_raw, int parts, void* stream);
int aldm_groupnorm_split_f16(const float* x1, const float* x2, int B, int P, int C1, int C2, int G, float eps,
                             const float* gamma, const float* beta, int act, float* scale, float* shift, float* ws,
                             void* dst, void* dst_raw, int raw_parts, float f16_scale, void* stream);
/* LayerNorm over the last dim of [M, C] (attention.py:393-395), eps 1e-5                   */
int aldm_layernorm(const float* x, float* y, int M, int C, const float* gamma,
                   const float* beta, float eps, void* stream);
/* same, writing the result as a split image (y_split, C % 32 == 0) and optionally also as fp32 (y may be NULL)    */
int aldm_layernorm_split(const float* x, float* y, void* y_split, int M, int C, const float* gamma,
                         const float* beta, float eps, int parts, void* stream);
int aldm_layernorm_split_f16(const float* x, float* y, void* y_split, int M, int C, const float* gamma,
                             const float* beta, float eps, float f16_scale, void* stream);

/* ---- attention ------------------------------------------------------------------------ */
/* Multi-head attention, head dim 32, flash-style online softmax on fp32 MFMA:
 *   out[b, i, h*32:(h+1)*32] = softmax_j(scale * q_i.k_j  [masked -> -FLT_MAX]) @ v
 * attention.py:343-367.  q/k/v/out are [B, L, *] with independent row pitches so a fused
 * QKV projection buffer can be consumed in place.  mask: [B, Lk] floats (1 = keep) or NULL
 * (attention.py:357-361: masked scores are set to -finfo.max, NOT -inf).                   */
int aldm_attention_d32(const float* q, const float* k, const float* v, float* out,
                       int B, int heads, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo,
                       const float* mask, float scale, void* stream);
/* same, writing the result (also / only: out may be NULL) as a split image with heads*32 channels per row — the
 * pre-split A operand of the to_out projection (attention.py:366)                                               */
int aldm_attention_d32_split(const float* q, const float* k, const float* v, float* out, void* out_split,
                             int parts, int B, int heads, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo,
                             const float* mask, float scale, void* stream);
/* Self-attention over the pre-split K / V^T images an ALDM_EPI_QKV launch wrote (ABI v6): q fp32 [B, Lq, *] (row pitch ldq),
 * k_split / vt_split as described at ALDM_EPI_QKV with `parts` parts, no mask; out / out_split as aldm_attention_d32_split.
 * Any Lk (ABI v10): with Lk % 32 != 0 the last key tile is partial — its keys >= Lk are masked (their k_split rows lie outside
 * the (sample, head) buffer descriptor and read as 0: no rows past the image are needed) and schedule 1 runs
 * whatever aldm_attention_sched says; the same holds for aldm_attention_d32_presplit_f16.  `parts` must match the attention
 * mode in force (2 for bf16x3, 3 for bf16x6).                                                                            */
int aldm_attention_d32_presplit(const float* q, const void* k_split, const void* vt_split, float* out, void* out_split,
                                int parts, int B, int heads, int Lq, int Lk, int ldq, int ldo, float scale, void* stream);
/* Ragged token counts (ABI v10): src = the v^T image of an ALDM_EPI_QKV launch over B * L rows with qkv_rows = B * L rounded up
 * to 32 ([heads][ceil(B L / 32)][parts][32][32] bf16 / fp16); dst = the per-sample image [B][heads][ceil(L / 32)][parts][32][32]
 * aldm_attention_d32_presplit{,_f16} reads, the last tile's keys >= L zero.                                                  */
int aldm_vt_regroup(const void* src, void* dst, int B, int L, int heads, int parts, void* stream);
/* Matrix-core path of aldm_attention_d32, PROCESS wide: 1 = fp32 MFMA, 2 = "bf16x6" (both products as 6 bf16 partial
 * products of exact 3-part operand splits), 3 = "bf16x3" ((hi, mid) rounded to nearest, 3 partial products), -1 =
 * default: $ALDM_ATTN_MMA if set, else the engine's $ALDM_MMA, else bf16x6 ("f32" | "bf16x6" | "bf16x3"; anything else is
 * reported on stderr and ignored).  Returns the previous mode; other values only query.                         */
int aldm_attention_mma(int mode);
/* Schedule of aldm_attention_d32_presplit (tests / tools; process wide): -1 = default ($ALDM_ATTN_SCHED, else 1), 0 = the round-3/4
 * pipelined kernel, 1 = the re-scheduled exact-max loop (bitwise the fp32-K/V path), 2 = the one-pass loop with a fixed softmax
 * reference per row (opt-in experiment, 1.7x the error), 3 = K / V^T tiles shared by a block's waves through LDS (ABI v9).
 * Returns the previous setting; other values only query.                                                                  */
int aldm_attention_sched(int sched);
/* Query tiles per wave (1 | 2) that every attention launcher above picks for this (B, heads, Lq) (ABI v13; host only, no launch):
 * 2 = 64 queries per wave and 256 per block, taken when Lq >= 128 and ceil(Lq / 256) * heads * B >= 128; $ALDM_ATTN_QT (read
 * once) overrides.  For tests, which reach either kernel family by shape and assert here which one they reached.          */
int aldm_attention_query_tiles(int B, int heads, int Lq);
/* "f16x3" self-attention (ABI v9): k_split / vt_split are the 2-part fp16 images an ALDM_EPI_QKV launch with out_split_fmt =
 * ALDM_FMT_F16 wrote (of k_scale * k and v_scale * v); q is split in the kernel into fp16 parts of q_scale * scale * log2(e) * q
 * (the caller vouches for |q_scale * scale * log2(e) * q| <= 65504: a LayerNorm-fed projection is bounded by R c), the
 * probabilities into fp16 parts of 2^15 p; Q.K^T and P.V run hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (24 matrix
 * instructions per 32-key tile and 64 queries instead of 48).  The softmax reference is the integer ceiling of the running
 * maximum in log2 units, so its offsets are exact.  out_split (optional): a bf16 image with out_parts (2 | 3) parts, or with
 * out_parts = 0 the 2-part fp16 image of out_scale * out (|out| <= max|v|: out_scale = v_scale is always safe) — the operand
 * of a three-product to_out projection.                                                                                   */
int aldm_attention_d32_presplit_f16(const float* q, const void* k_split, const void* vt_split, float* out, void* out_split,
                                    int out_parts, float out_scale, int B, int heads, int Lq, int Lk, int ldq, int ldo,
                                    float scale, float q_scale, float k_scale, float v_scale, void* stream);
/* ---- folded cross-attention on a short context (ABI v21) ----------------------------------------------------------------
 * The context of a cross-attention sublayer is fixed for a whole sampling run, so with Lk <= 8 keys the two C x C projections
 * around the attention fold into two per-sample operands, once per job (N = heads * 8 score columns, column n = head * 8 + key,
 * Np = N rounded up to 32; key columns >= Lk and the columns >= N are zero):
 *   Mq_b[c, n] = 32^-1/2 log2(e) sum_d Wq[head*32 + d, c] k_b[key, head*32 + d]        (C x Np; scores come out in log2 units)
 *   Mo_b[n, c] = sum_d v_b[key, head*32 + d] Wout[c, head*32 + d]                      (Np x C)
 *   out = softmax_per_head(LayerNorm(h) Mq_b, mask) Mo_b + b_out + h
 * aldm_xattn_fold_prepare writes both as 3-part bf16 images (every entry a 32-term dot product accumulated in fp64, rounded ONCE
 * to fp32, then split exactly: x = hi + mid + lo), in the order the kernel's matrix instructions take them — one 16-byte piece =
 * one lane's operand fragment (lane l: r = l & 31, u = l >> 5; element j = 0..7), 1 KiB per (tile, k-step, part):
 *   mq_img: [b][n tile = Np/32][k step = C/16][part 0..2][lane 64][8] bf16, element = Mq_b[16 kstep + 8 u + j, 32 ntile + r]
 *   mo_img: [b][c tile = C/32][n step = Np/16][part 0..2][lane 64][8] bf16, element = Mo_b[16 nstep + 8 u + j, 32 ctile + r]
 * aldm_xattn_fold_bytes = the size of either image (they are equally large).  kv: the cached projection [B, Lk, 2C] (k | v);
 * wq / wout: to_q.weight / to_out[0].weight, [C, C] row-major fp32.  The images are the caller's: a second prepare into the
 * same buffers refreshes them in place.
 * aldm_xattn_folded is the sublayer in one launch: h, out [B*L, C] fp32 (out must not alias h), mask [B, Lk] (a key takes part
 * iff its entry == 1; masked keys score -FLT_MAX like aldm_attention_d32, so a row with every key masked is uniform over the
 * Lk real keys) or NULL.  Needs C % 32 == 0, heads * 32 == C, 1 <= Lk <= 8, L % 32 == 0, and C <= 640: a block keeps its
 * rows and probabilities as 3-part images in the 160 KiB LDS.
 * aldm_xattn_fold_plan (host only, like aldm_groupnorm_plan): the launch geometry of a shape — tile_rows (32 | 64 rows of ONE
 * sample per block), col_splits (blocks that share a row tile, each recomputing the scores and writing C / col_splits output
 * columns), waves per block, blocks, lds_bytes.  Returns 0 when the kernel does not support the shape, 1 when it does but the
 * measured in-step gate (docs/experiments_r1-r6.md §10.8) keeps the unfolded path for it, 2 when the step should use it.  Out
 * pointers may be NULL.                                                                                                      */
int aldm_xattn_fold_plan(int B, int L, int C, int heads, int Lk, int* tile_rows, int* col_splits, int* waves, int* blocks,
                         int* lds_bytes);
int64_t aldm_xattn_fold_bytes(int B, int C);
int aldm_xattn_fold_prepare(const float* kv, const float* wq, const float* wout, void* mq_img, void* mo_img, int B, int C,
                            int heads, int Lk, void* stream);
int aldm_xattn_folded(const float* h, float* out, const float* gamma, const float* beta, float eps, const void* mq_img,
                      const void* mo_img, const float* b_out, const float* mask, int B, int L, int C, int heads, int Lk,
                      void* stream);
/* Windowed relative-position self-attention of the VITS phoneme encoder (phoneme_encoder/attentions.py:239-289,
 * window_size = `window` <= 8, shared heads): per head h (channels [h*d, (h+1)*d), d <= 128)
 *   s[i, j] = (q_i/sqrt(d)).k_j + [|j-i| <= window] (q_i/sqrt(d)).emb_k[j-i+window];  s = -1e4 where mask_i*mask_j == 0;
 *   out_i = softmax_j(s) v + sum_r p[i, i+r-window] emb_v[r].   q/k/v/out: [B, T, *] rows with pitches ld*; emb_*:
 * [2*window+1, d]; mask [B, T] (1 = token).  Exact fp32 FMA (a once-per-prompt conditioner, latency bound).       */
int aldm_rel_attention(const float* q, const float* k, const float* v, float* out, int B, int heads, int T, int d,
                       int ldq, int ldk, int ldv, int ldo, const float* emb_k, const float* emb_v, int window,
                       const float* mask, void* stream);
/* y[r, c] = x[r, c] * s[r] (+ res[r, c] when res != NULL): the x * x_mask of the encoder's conv FFN
 * (attentions.py:406-413) and the final + positional embedding (encoders/modules.py:103); divide != 0:
 * y = x / max(s[r], 1e-12) (F.normalize with s = row norms: CLAP embeddings, clap/open_clip/model.py:745)           */
int aldm_rowscale_add(const float* x, const float* s, const float* res, float* y, int64_t rows, int C, int divide,
                      void* stream);
/* T5LayerNorm (FLAN-T5 conditioner, encoders/modules.py:173-198 via transformers): y = weight * x * rsqrt(mean(x^2) + eps) */
int aldm_rmsnorm(const float* x, float* y, int M, int C, const float* weight, float eps, void* stream);
/* Row softmax of attention scores [B, heads, q_rows, N] with an additive bias [heads, q_rows, N] shared by the batch (T5's
 * bucketed relative-position bias) and a key padding mask [B, N] (0 = padded key: weight 0, the reference adds finfo.min) */
int aldm_softmax_rows_bias(const float* x, float* y, int B, int heads, int q_rows, int N, float scale, const float* bias,
                           const float* keymask, void* stream);
/* row softmax with pre-scale: y = softmax(scale * x) over the last dim of [M, N]
 * (model.py:220-221)                                                                        */
int aldm_softmax_rows(const float* x, float* y, int64_t M, int N, float scale, void* stream);
/* Causal + key-padding masked row softmax for attention score rows laid out [B, heads, q_rows, N] (GPT-2 blocks of the
 * AudioMAE-token sequence generator, audiomae_gen/sequence_input.py:308-323 via transformers GPT2Attention): key j of
 * batch b takes part iff keymask[b, j] != 0 and j <= q_pos0 + i for query row i; excluded keys get weight 0.       */
int aldm_softmax_rows_masked(const float* x, float* y, int B, int heads, int q_rows, int N, float scale,
                             const float* keymask, int q_pos0, void* stream);

/* ---- single-position decode step of the GPT-2 sequence generator (ABI v7) ----------------------------------------------
 * audiomae_gen/sequence_input.py:294-325 calls transformers' GPT2Model once per generated AudioMAE token (512 dependent calls for
 * the speech model, 8 for text-to-audio); with a key/value cache each call is ONE new position per sample: M = batch <= 16 rows
 * through every Linear.  At that M the layers are weight streams, not matrix-core work, and the general path spends its time in
 * launches (~17 per GPT-2 block).  These two entry points are the decode step's layer body in 5 launches per block.
 *
 * aldm_decode_linear: y[M, N] = act(LN(x)[M, K] . W[K, N] + bias) + res — transformers Conv1D (weight stored [in, out] = [K, N],
 *   used as is, fp32) with the preceding LayerNorm (ln_gamma / ln_beta both NULL: none; statistics over the whole row, biased
 *   variance, eps inside the root; K <= 1024 then) and the following activation (ALDM_ACT_NONE | GELU | GELU_TANH | SILU | TANH) /
 *   residual add fused.  1 <= M <= 16; K a multiple of 64 * ceil(K / 1024).  Exact fp32 FMA in a fixed order (deterministic,
 *   no workspace): one block per 32 output columns sums all of K.                                                            */
int aldm_decode_linear(const float* x, int ldx, int M, int K, const float* w_kn, int N, const float* bias,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, int act, const float* res, int ldr,
                       float* y, int ldy, void* stream);
/* aldm_decode_attention: attention of the new position over the key/value cache (transformers GPT2Attention._attn with
 *   layer_past, head dim 64): qkv [B, 3E] = the c_attn output rows (q | k | v, E = heads * 64) of the new position; *pos (a
 *   DEVICE int64, so a captured graph advances it) = its cache slot.  Writes k / v into k_cache / v_cache
 *   [B * heads, n_tot, 64] at slot *pos, scores q.k_j * scale against every key j <= *pos with keymask[b, j] != 0 (the caller
 *   switches slot *pos on first; slots behind it are not part of the sequence yet), softmax, P.V; out [B, E] head-merged.
 *   n_tot <= 1024 (GPT-2's n_positions).                                                                                     */
int aldm_decode_attention(const float* qkv, int ldq, const int64_t* pos, float* k_cache, float* v_cache, const float* keymask,
                          int B, int heads, int n_tot, float scale, float* out, int ldo, void* stream);
/* ---- the same decode step on the whole chip (ABI v9, round 6): 7 launches per GPT-2 block -----------------------------------
 * aldm_decode_linear gives one block all of K for its 32 columns: 24 - 96 blocks per launch, each streaming 96 - 393 KB of
 * weights through one compute unit's memory path.  These entry points cut K into S slices so that every launch covers the chip
 * with one HBM round trip per block, and hand the partial sums to the NEXT launch instead of reducing them across blocks:
 *
 * aldm_decode_gemv_slices(K, N): the S the library uses for a [K, N] weight (K / S rows per slice, a multiple of 32, <= 512;
 *   column tiles x S >= 256 blocks where K allows) — the caller sizes ypart [S, M, N] with it; 0 = K cannot be sliced.
 * aldm_decode_gemv: ypart[s][m][n] = sum over slice s of xe[m][k] W[k][n], W = Conv1D's own [K, N] fp32 weight (non-temporal
 *   loads: read once per token), xe = xact(xbias + x[0] + x[1] + ... + x[xparts-1]) with x[j] = x + j * xstride (partial slabs
 *   [M, ldx] of the previous aldm_decode_gemv, summed in slab order; xparts = 1, xbias = NULL, xact = NONE: plain rows).
 * aldm_decode_reduce_ln: per row m: v = part[0][m] + ... + part[nparts-1][m] (slab order; nparts = 0: none) + bias (row
 *   *bias_row of a [rows, N] table when bias_row != NULL — GPT-2's position embedding at a DEVICE-side position) + res;
 *   h_out = v (may alias res; NULL: not stored); with ln_gamma: xn (and xn2 when != NULL) = LayerNorm(v) gamma + beta
 *   (mean, then the centred second moment, biased variance, eps inside the root).  N <= 1024, N % 4 == 0.
 * aldm_decode_attention_parts: aldm_decode_attention with q | k | v = qbias + the qparts slabs of a sliced c_attn.
 * Deterministic (fixed slab order), no atomics, no workspace besides the slabs the caller owns.                           */
int aldm_decode_gemv_slices(int K, int N);
int aldm_decode_gemv(const float* x, int ldx, int xparts, int64_t xstride, const float* xbias, int xact, int M, int K,
                     const float* w_kn, int N, float* ypart, void* stream);
int aldm_decode_reduce_ln(const float* part, int nparts, int64_t pstride, int ldp, const float* bias, const int64_t* bias_row,
                          const float* res, int ldr, int M, int N, float* h_out, int ldh, const float* ln_gamma,
                          const float* ln_beta, float ln_eps, float* xn, int ldn, float* xn2, int ldn2, void* stream);
int aldm_decode_attention_parts(const float* qkv_part, int ldq, int qparts, int64_t qstride, const float* qbias,
                                const int64_t* pos, float* k_cache, float* v_cache, const float* keymask, int B, int heads,
                                int n_tot, float scale, float* out, int ldo, void* stream);

/* ---- elementwise ---------------------------------------------------------------------- */
/* GEGLU gate: y[m, c] = x[m, c] * gelu_erf(x[m, C + c]), x: [M, 2C] (attention.py:42-44)   */
int aldm_geglu(const float* x, float* y, int64_t M, int C, void* stream);
/* sinusoidal timestep embedding [cos | sin], util.py:172-196; t: [B] floats               */
int aldm_timestep_embedding(const float* t, float* out, int B, int dim, float max_period,
                            void* stream);
/* NCHW <-> NHWC (the reference's rearrange at attention.py:462,465 disappears; only the
 * 8/16-channel latent crosses layouts at the UNet boundary). rep: write `rep` copies.     */
int aldm_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, int rep, void* stream);
int aldm_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, void* stream);
/* Fused classifier-free guidance + DDIM step (ddim.py:298-355).  eps holds [e_uncond ; e_cond]
 * ([2, n] when cfg != 0 path is used, else [1, n]); coef (device) = {sqrt(1-a_t), sqrt(a_t),
 * sqrt(1-a_prev-sigma^2), sqrt(a_prev), sigma_t, guidance_scale, use_cfg, 0}.
 *   e = e_u + s*(e_c - e_u); pred_x0 = (x - c0*e)/c1; x_prev = c3*pred_x0 + c2*e + c4*noise  */
int aldm_ddim_step(const float* x, const float* eps, const float* noise, const float* coef,
                   float* x_prev, float* pred_x0, int64_t n, void* stream);
/* The same step with its inputs selected on the DEVICE (ABI v6): coef = coef_tab[*step_idx] (rows of coef_ld >= 7 floats),
 * noise = noise_tab[*step_idx] (rows of n floats), x updated IN PLACE (x_prev overwrites x).  Together with
 * aldm_step_advance it lets one captured HIP graph serve every DDIM step with no host-issued copy between replays.   */
int aldm_ddim_step_indexed(float* x, const float* eps, const float* noise_tab, const float* coef_tab,
                           const int* step_idx, float* pred_x0, int64_t n, int coef_ld, void* stream);
/* PLMS (plms.py:261-360; ABI v11).  sigma = 0 (make_schedule refuses any other eta): no noise operand.  eps / e_t / e_next hold
 * [e_uncond ; e_cond] ([2, n]) when coef[6] != 0, else [1, n]; coef rows as in aldm_ddim_step (coef[4] unused).  The history ring
 * hist[3, n] keeps the model output of step j — after the guidance combine, before the multistep combine — in slot j % 3.
 * aldm_plms_first_step, step 0 (pseudo improved Euler): e_next == NULL writes the provisional x_out = update(x, e_t) and pred_x0
 * (hist untouched, may be NULL); with e_next, e' = (e_t + e_next) / 2, x_out = update(x, e'), hist[0] = e_t.  x_out may be x.
 * aldm_plms_step_indexed, steps >= 1, in place on x: s = *step_idx, coef = coef_tab[s], order k = min(s, 3),
 *   e' = (3 e - h1) / 2 | (23 e - 16 h1 + 5 h2) / 12 | (55 e - 59 h1 + 37 h2 - 9 h3) / 24   with h_j = hist[(s - j) % 3],
 *   pred_x0 = (x - c0*e')/c1; x = c3*pred_x0 + c2*e'; hist[s % 3] = e.   A launch that finds s == 0 writes nothing.
 * With aldm_step_advance one captured HIP graph serves every step >= 1 (ring slots follow the counter: no host rotation).   */
int aldm_plms_first_step(const float* x, const float* e_t, const float* e_next, const float* coef_row, float* x_out,
                         float* pred_x0, float* hist, int64_t n, void* stream);
int aldm_plms_step_indexed(float* x, const float* eps, float* hist, const float* coef_tab, const int* step_idx,
                           float* pred_x0, int64_t n, int coef_ld, void* stream);
/* DPM-Solver++(2M), deterministic, data-prediction form (Lu et al. 2022, Algorithm 2; ABI v12), in place on x.  s = *step_idx,
 * coef = coef_tab[s] (rows of coef_ld >= 7 floats) = {sigma_t, alpha_t, sigma_prev/sigma_t, -alpha_prev*expm1(-h), w, guidance_scale,
 * use_cfg} with alpha = sqrt(abar), sigma = sqrt(1 - abar), h = lambda_prev - lambda_t, lambda = log(alpha/sigma), w = 1/(2r),
 * r = h_last/h; w == 0 marks a first-order step.  eps holds [e_uncond ; e_cond] ([2, n]) when coef[6] != 0, else [1, n].
 *   e = e_u + s*(e_c - e_u); x0 = (x - c0*e)/c1; D = x0 (w == 0) | x0 + w*(x0 - x0_buf); x = c2*x + c3*D; x0_buf = x0.
 * x0_buf[n] is the one-slab history and the pred_x0 output; at w == 0 its old content is not read (it may be uninitialised).
 * The counter is not range-checked, as in aldm_ddim_step_indexed: aldm_step_advance saturates it at the last row.           */
int aldm_dpmpp_step_indexed(float* x, const float* eps, float* x0_buf, const float* coef_tab, const int* step_idx, int64_t n,
                            int coef_ld, void* stream);
/* DPM-Solver++(2M) SDE (Lu et al. 2022, the SDE variant in its midpoint form, generalised by eta in [0, 1]; ABI v26),
 * in place on x.  s = *step_idx, coef = coef_tab[s] (rows of coef_ld >= 9 floats): columns 0-7 are exactly what
 * aldm_dpmpp_step_indexed reads — {sigma_t, alpha_t, c2, c3, w, guidance_scale, use_cfg, phi} — with
 *   c2 = (sigma_prev/sigma_t) exp(-eta h),  c3 = -alpha_prev expm1(-(1 + eta) h),  and column 8:  c4 = sigma_prev sqrt(-expm1(-2 eta h)).
 *   e, x0, D as in aldm_dpmpp_step_indexed;  x = (c2*x + c3*D) + c4*z;  x0_buf = x0
 * z = row clamp(s, 0, noise_rows - 1) of noise_tab [noise_rows, n], the step's unit noise (already scaled by a temperature): whatever
 * the counter holds, the launch stays inside the table.  The coefficient row itself is not range-checked, as in
 * aldm_dpmpp_step_indexed.  fp32, the formula's operation order, c4*z and the last sum rounded separately (no contraction): bitwise
 * reproducible.  When c4 == 0 the noise element is not loaded — a NaN table cannot reach x — and the launch is bitwise
 * aldm_dpmpp_step_indexed on the same first eight columns; when w == 0 the history slab is not loaded.  16-byte accesses when
 * n % 4 == 0 and x, eps, x0_buf and noise_tab are 16-byte aligned (every row is then), else a scalar form; grid-stride, 64-bit
 * indexing.  Refused before any launch: null pointers, n <= 0, noise_rows < 1, coef_ld < 9, x or x0_buf overlapping the noise table.
 * No atomics, nothing kept between launches.                                                                                      */
int aldm_dpmpp_sde_step_indexed(float* x, const float* eps, float* x0_buf, const float* noise_tab, int noise_rows,
                                const float* coef_tab, const int* step_idx, int64_t n, int coef_ld, void* stream);
/* Classifier-free guidance combine with guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are
 * Flawed", section 3.4; ABI v14).  s = step_idx ? *step_idx : 0, coef = coef_tab[s] (rows of coef_ld >= 8 floats): coef[5] the
 * guidance scale g, coef[7] = phi.  eps holds [e_uncond ; e_cond] as [2, B, n_s]; per sample b over its n_s elements:
 *   e_g = e_u + g*(e_c - e_u); f = phi * std(e_c) / std(e_g) + (1 - phi); out[b] = f * e_g.
 * f = 1 when std(e_g) == 0 or n_s == 1 (the textbook form gives NaN there).  Two-pass statistics in fp32 in a fixed order: results
 * are bitwise reproducible.  One launch, one workgroup per sample.  out [B, n_s] must not overlap eps; eps and coef_tab are not
 * written; a non-finite input reaches every output of its sample and no other sample.  A step kernel then takes out as its
 * [1, n] model output (coef[6] == 0).                                                                                            */
int aldm_cfg_rescale_indexed(const float* eps, float* out, const float* coef_tab, const int* step_idx, int B, int64_t n_s,
                             int coef_ld, void* stream);
/* Composable guidance (Liu et al. 2022, "Compositional Visual Generation with Composable Diffusion Models"; ABI v27):
 * the K+1 predictions of one UNet pass reduced to the standard [uncond ; cond] pair, one launch behind the pass.  eps holds
 * [(K+1), n]: group 0 the unconditional prediction, groups 1..K the prompts'.  w_tab holds [rows, K+1] floats: column 0 is
 * c_0 = 1 - sum_k w_k (formed in fp64 on the host, rounded once), columns 1..K are c_k = w_k.  r = clamp(step_idx ? *step_idx : 0,
 * 0, rows - 1) — the blend-gather entries' conventions for the counter.  The row's coefficients are read once per thread.
 *   e_c[i] = sum_g c_g * eps[g*n + i]   over ascending g,   == e_u + sum_k w_k (e_k - e_u)
 * A group whose coefficient is exactly 0 is skipped before its element is loaded (a NaN there cannot reach the output, and it costs no
 * traffic); the first kept term is a plain multiply, every later one one fused multiply-add; no kept term gives 0.  K = 1, w = 1
 * makes e_c bitwise eps[1].  pair == 1: out[0:n] = eps[0] bitwise, out[n:2n] = e_c — the pair every step kernel,
 * aldm_cfg_rescale_indexed and the window merge take.  pair == 0 (no guidance): out[0:n] = e_c.  out == eps is allowed (in place: a
 * thread owns element i of every group and stores after it has loaded them all; group 0 is not rewritten under pair == 1); any other
 * overlap of out with eps, and any overlap of out with w_tab, is refused.  16-byte accesses when n % 4 == 0 and eps and out are
 * 16-byte aligned, else a scalar form; grid-stride, 64-bit indexing; no atomics: the result does not depend on the launch geometry.
 * Refused before any launch: null eps / out / w_tab, K outside [1, ALDM_MAX_COMPOSE], rows < 1, pair outside {0, 1}, n outside
 * (0, 2^40], the overlaps above.                                                                                                  */
#define ALDM_MAX_COMPOSE 8
int aldm_cfg_compose_indexed(const float* eps, float* out, const float* w_tab, const int* step_idx, int rows, int K, int pair,
                             int64_t n, void* stream);
/* *step_idx += 1 and t_cur[0..nt) = t_tab[min(*step_idx, steps-1)] (the next step's timestep row, the UNet's static input;
 * the time_range of ddim.py:205-213 stored as floats, one row per step in loop order)                                  */
int aldm_step_advance(int* step_idx, const float* t_tab, float* t_cur, int nt, int steps, void* stream);
/* Ancestral DDPM step (LatentDiffusion.sample -> p_sample, ddpm.py:357-373,1127-1181), reference
 * operation order: x_recon = a*x - b*eps; mean = c1*x_recon + c2*x; x_prev = mean + s*noise with
 * coef (device) = {sqrt(1/abar_t), sqrt(1/abar_t - 1), posterior_mean_coef1, posterior_mean_coef2,
 * nonzero_mask*exp(0.5*posterior_log_variance_clipped)}.                                        */
int aldm_ddpm_step(const float* x, const float* eps, const float* noise, const float* coef,
                   float* x_prev, int64_t n, void* stream);
/* Inpainting blend, in place on x (ddim.py:226-231, q_sample ddpm.py:430-436):
 *   x = (sa*x0 + so*qnoise)*mask + (1 - mask)*x,  coef (device) = {sqrt(abar_t), sqrt(1 - abar_t)} */
int aldm_inpaint_blend(const float* x0, const float* qnoise, const float* mask, const float* coef,
                       float* x, int64_t n, void* stream);
/* The forward jump of resampled inpainting (RePaint, Lugmayr et al. 2022, section 4.2; ABI v23), in place on x:
 *   s = step_idx ? *step_idx : 0;  x[i] = c0*x[i] + c1*noise_tab[s*n + i],  c0 = coef_tab[s*coef_ld], c1 = coef_tab[s*coef_ld + 1]
 * with {c0, c1} = {sqrt(rho), sqrt(1 - rho)}, rho = abar(k') / abar(k) < 1: q(x_k' | x_k) of the forward process over the whole jump,
 * one launch per jump.  fp32, two rounded products and one rounded sum in that order (no contraction): bitwise reproducible.  It reads
 * the step graph's own counter, noise table and coefficient table (rows of coef_ld >= 2 floats) and is followed by
 * aldm_step_advance; the step graph itself is untouched.  The counter is not range-checked, as in aldm_ddim_step_indexed:
 * aldm_step_advance saturates it at the last row.  x may not overlap noise_tab (checked against its first row: the row count does
 * not cross this ABI).  No atomics, nothing kept between launches.                                                              */
int aldm_renoise_indexed(float* x, const float* noise_tab, const float* coef_tab, const int* step_idx, int64_t n, int coef_ld,
                         void* stream);
/* Graded keep levels (differential diffusion, Levin & Fried 2023, "change maps"; ABI v24): the binary mask a step's
 * blend reads, rewritten per step from a map of levels in [0, 1]:
 *   r = clamp(step_idx ? *step_idx : 0, 0, rows - 1);  mask[i] = level[i] > thr_tab[r] ? 1.0f : 0.0f
 * — the blend-gather entries' conventions for the counter (negative: row 0, past the end: the last row, null: row 0).  thr_tab holds
 * `rows` floats, one per visit of the run (sampling.keep_thresholds: i / S).  Exactly the bit patterns of 0.0f and 1.0f are written;
 * the comparison is ordered, so a NaN level gives 0 and equality releases the frame.  The counter is read, never written.  16-byte
 * accesses when n % 4 == 0 and level and mask are 16-byte aligned, else a scalar path.  Refused before any launch: null pointers,
 * n <= 0, rows <= 0, mask overlapping level (in place would destroy the levels).  No atomics, nothing kept between launches.       */
int aldm_keep_threshold_indexed(const float* level, const float* thr_tab, const int* step_idx, int rows, float* mask, int64_t n,
                                void* stream);
/* VAE posterior sample fused with the forward diffusion to the sampler's first noise level (audio-to-audio; ABI v16): one launch
 * from the encoder's channels-last moments (autoencoder.py:103-109, distributions.py:24-41, ddpm.py:793-802, ddim.py:434-449):
 *   moments_cl [B0, hw, 2C] channels-last: mean = channels 0..C-1, logvar = channels C..2C-1
 *   n_post [B0, C, hw] NCHW, the posterior noise;  n_enc [B0*n_gen, C, hw] NCHW, the forward-diffusion noise
 *   coef (device) = {scale_factor, sqrt(abar), sqrt(1 - abar)}
 *   lv = clamp(logvar, -30, 20); std = expf(0.5f*lv); z = scale*(mean + std*n_post); x_t[r] = sqrt(abar)*z[r % B0] + sqrt(1 - abar)*n_enc[r]
 * z [B0, C, hw] and x_t [B0*n_gen, C, hw] are NCHW; rows of x_t are candidate-major (torch.cat([z]*n_gen)).  A NaN logvar stays NaN
 * (torch.clamp's behaviour), +-inf clamp to 20 / -30.  C % 4 == 0, moments_cl 16-byte aligned; bad arguments are refused before
 * the launch.                                                                                                                    */
int aldm_posterior_qsample(const float* moments_cl, const float* n_post, const float* n_enc, const float* coef, float* z,
                           float* x_t, int B0, int n_gen, int C, int64_t hw, void* stream);
/* Windowed (long-form) diffusion, ABI v18: a long latent [B, C, T, F] is denoised through W overlapping windows of
 * Tw frames along T.  The window starts are passed BY VALUE, so a captured step graph carries them as kernel arguments: no device
 * table, no copy inside a capture.  Both entries check them on the host before the launch: n == W <= ALDM_MAX_WINDOWS, s[0] == 0,
 * strictly ascending with gaps <= Tw (every frame has a window), s[n-1] == T - Tw.                                               */
#define ALDM_MAX_WINDOWS 32
typedef struct aldm_window_starts {
    int n;
    int s[ALDM_MAX_WINDOWS];
} aldm_window_starts;
/* win[(j*B + b), c, p, f] = x[b, c, s_j + p, f]: x [B, C, T, F] -> win [W*B, C, Tw, F], window-major rows (the order in which a
 * conditioning is tiled for W windows).  A bit-exact copy; win must not overlap x.                                             */
int aldm_window_gather(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F,
                       void* stream);
/* The tapered, normalised overlap-add of window-wise tensors: win [H, W*B, C, Tw, F], wn [W, Tw] (the normalised weights: over
 * every frame they sum to 1) -> out [H, B, C, T, F]; H = 1, or 2 for the [uncond ; cond] pair of a guided UNet pass.
 *   out[h, b, c, t, f] = sum over the windows j with s_j <= t < s_j + Tw, in ascending j, of wn[j, t - s_j] * win[h, j*B + b, c, t - s_j, f]
 * in fp32: the first term a plain multiply, every later term one fmaf.  Gather form, no atomics: bitwise reproducible and
 * independent of the launch geometry; a frame under one window with wn == 1 reproduces its input bit for bit; a non-finite input
 * reaches exactly the frames its window covers.  out must overlap neither win nor wn.  The same entry cross-fades window-wise VAE
 * decodes in the mel domain (C = 1, F = mel bins, the plan scaled by the VAE's time factor).                                    */
int aldm_window_merge(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W, int C, int T,
                      int Tw, int F, void* stream);
/* The inpainting blend on the long latent fused with the window gather (ABI v19): one launch per step of a windowed
 * run that keeps a source.  s = step_idx ? *step_idx : 0; the q-noise row is qnoise[min(s, q_rows-1)] of [q_rows, B, C, T, F], the
 * coefficients blend_coef[min(s, coef_rows-1)] of [coef_rows, 2] = {sa = sqrt(abar_t), so = sqrt(1 - abar_t)} (q_rows == 1: one
 * staged draw per step).  In place on x, then every window copy of the blended value:
 *   x[b,c,t,f] = (sa*x0 + so*qn)*m + (1 - m)*x;   win[(j*B + b), c, t - s_j, f] = x[b,c,t,f] for every j with 0 <= t - s_j < Tw
 * mask, x0 [B, C, T, F].  Scatter form: one thread owns a long-latent element, every window element has one writer and all are
 * written; no atomics.  The expression and its order are aldm_inpaint_blend's: the launch is bitwise aldm_inpaint_blend followed by
 * aldm_window_gather.  win may overlap none of x, x0, qnoise, mask; x none of x0, qnoise, mask; checked before the launch.        */
int aldm_window_blend_gather(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                             const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_starts starts, int B, int W,
                             int C, int T, int Tw, int F, void* stream);
/* Ring plans (seamless loops), ABI v20: the T frames are a circle and window j covers the frames (s_j + p) mod T, p in
 * [0, Tw), so a window may wrap from frame T-1 to frame 0 and the junction of end and start lies inside a window.  The three entries
 * below are the wrap-around forms of aldm_window_gather, aldm_window_merge and aldm_window_blend_gather, with their siblings'
 * argument lists, operation order and aliasing rules; the linear entries are unchanged.  The starts are checked on the host before
 * the launch: n == W, 2 <= W <= ALDM_MAX_WINDOWS, s[0] == 0, strictly ascending and < T, every gap — the wrap gap T - s[W-1]
 * included — <= Tw (every frame has a window), Tw <= T (no window covers a frame twice).  The wrap is along T: a 16-byte access
 * along F never straddles it; it costs a compare and a subtract, no integer modulo.                                              */
/* win[(j*B + b), c, p, f] = x[b, c, (s_j + p) mod T, f], a bit-exact copy: per (b, c) at most two contiguous spans of x. */
int aldm_window_gather_ring(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F,
                            void* stream);
/* out[h, b, c, t, f] = sum over the windows j, ascending, with p = (t - s_j) mod T < Tw, of wn[j, p] * win[h, j*B + b, c, p, f]:
 * the first term a plain multiply, every later one one fmaf; H = 1 | 2; gather form, no atomics.  wn: the ring plan's weights,
 * normalised by the circular sum of the tapers, so the output is periodic by construction.                                       */
int aldm_window_merge_ring(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W, int C,
                           int T, int Tw, int F, void* stream);
/* aldm_window_blend_gather on a ring: in place x = (sa*x0 + so*qn)*m + (1 - m)*x, then win[(j*B + b), c, (t - s_j) mod T, f] = x
 * for every window j that covers t.  Every window element has exactly one writer.  Bitwise aldm_inpaint_blend followed by
 * aldm_window_gather_ring.                                                                                                        */
int aldm_window_blend_gather_ring(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                                  const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_starts starts, int B,
                                  int W, int C, int T, int Tw, int F, void* stream);
/* Moving window phases, ABI v25: a ring plan whose starts are all rotated, per step, by a phase the device-side step
 * counter selects — window j covers the frames (s_j + phi + p) mod T, p in [0, Tw).  A rigid rotation keeps every gap, so the ring
 * plan's weights wn hold for every phase.  The three entries below are siblings of the ring entries, which are unchanged.
 * `starts`: the ring plan's own, by value, checked on the host exactly as the ring entries check them.  `phase_tab`: a device table
 * of `rows` int32.  Row r = clamp(step_idx ? *step_idx : 0, 0, rows - 1) (aldm_keep_threshold_indexed's conventions; the counter is
 * read, never written) and phi = clamp(phase_tab[r], 0, T - 1): a value outside [0, T) CLAMPS, it does not wrap — whatever the table
 * holds, the launch stays inside its buffers; a caller reduces mod T on the host.  Host checks before every launch: the ring
 * entries' own, phase_tab != NULL, rows >= 1, the siblings' overlap rules, and phase_tab overlapping no written buffer.  With
 * phi == 0 each entry is bitwise its ring sibling.  16-byte accesses along F under the siblings' alignment rule.                   */
/* win == aldm_window_gather_ring of x rolled by -phi along T: win[(j*B + b), c, p, f] = x[b, c, (s_j + phi + p) mod T, f]. */
int aldm_window_gather_ring_phased(const float* x, float* win, aldm_window_starts starts, const int* phase_tab, const int* step_idx,
                                   int rows, int B, int W, int C, int T, int Tw, int F, void* stream);
/* out == aldm_window_merge_ring's result rolled by +phi along T, bit for bit: per output element the covering windows in ascending
 * j, the first term a plain multiply, every later one one fmaf; H = 1 | 2; gather form, no atomics.                               */
int aldm_window_merge_ring_phased(const float* win, const float* wn, float* out, aldm_window_starts starts, const int* phase_tab,
                                  const int* step_idx, int rows, int H, int B, int W, int C, int T, int Tw, int F, void* stream);
/* aldm_window_blend_gather_ring with rotated windows: x is left exactly as the ring sibling leaves it (the blend does not depend on
 * phi; step_idx selects the q-noise and coefficient rows as there, and the phase row), win == aldm_window_gather_ring of the blended
 * x rolled by -phi.  Every window element has exactly one writer and all are written; no atomics.                                 */
int aldm_window_blend_gather_ring_phased(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                                         const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_starts starts,
                                         const int* phase_tab, int rows, int B, int W, int C, int T, int Tw, int F, void* stream);
/* Prompt timelines, ABI v22: a ROW is one window under one prompt, so several rows may share a start.  The row starts
 * travel by value like the window starts; 64 of them (a two-minute clip with a scene every 10 s takes 35).  The three entries below
 * are siblings of aldm_window_gather, aldm_window_merge and aldm_window_blend_gather; those are unchanged and keep refusing repeated
 * starts.  Host checks before every launch: 1 <= n <= ALDM_MAX_ROWS, s[0] == 0, s non-decreasing, every increase <= Tw (every
 * frame has a row), s[n-1] == T - Tw, and the shape, overlap and pointer checks of the siblings.  Linear plans only.             */
#define ALDM_MAX_ROWS 64
typedef struct aldm_window_rows {
    int n;
    int s[ALDM_MAX_ROWS];
} aldm_window_rows;
/* win[(r*B + b), c, p, f] = x[b, c, s_r + p, f]: x [B, C, T, F] -> win [n*B, C, Tw, F], row-major; a bit-exact copy (rows that
 * share a start are equal copies).  win must not overlap x.                                                                      */
int aldm_window_gather_rows(const float* x, float* win, aldm_window_rows rows, int B, int C, int T, int Tw, int F, void* stream);
/* The weighted overlap-add of row-wise tensors: win [H, n*B, C, Tw, F], wr [n, Tw] (per-row, per-frame weights: taper times prompt
 * weight, normalised over the rows of a frame) -> out [H, B, C, T, F]; H = 1 | 2.
 *   out[h, b, c, t, f] = sum over the rows r with s_r <= t < s_r + Tw AND wr[r, t - s_r] != 0, in ascending r, of
 *                        wr[r, t - s_r] * win[h, r*B + b, c, t - s_r, f]
 * in fp32: the first kept term a plain multiply, every later one one fmaf; a frame where every covering row has weight 0 (no plan
 * of windows.row_plan has one) is written as 0.  A row of weight exactly 0 at a frame is SKIPPED there and its win element is not
 * loaded: a prompt contributes nothing outside its region, not even 0 * NaN; a frame under one row of weight 1 reproduces its
 * input bit for bit.  Gather form, no atomics.  out must overlap neither win nor wr.                                             */
int aldm_window_merge_rows(const float* win, const float* wr, float* out, aldm_window_rows rows, int H, int B, int C, int T, int Tw,
                           int F, void* stream);
/* aldm_window_blend_gather over rows: in place x = (sa*x0 + so*qn)*m + (1 - m)*x with the sibling's expression, operation order and
 * step-counter row selection, then win[(r*B + b), c, t - s_r, f] = x for every row r that covers t.  Every win element has exactly
 * one writer.  Bitwise aldm_inpaint_blend followed by aldm_window_gather_rows.                                                   */
int aldm_window_blend_gather_rows(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                                  const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_rows rows, int B, int C,
                                  int T, int Tw, int F, void* stream);
/* generic y = alpha*a + beta*b (b may be NULL) */
int aldm_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n,
               void* stream);
/* reflect padding of [B, T] by `pad` on both sides into rows of pitch ld_out (stft.py:60-64) */
int aldm_reflect_pad_1d(const float* x, float* y, int B, int T, int pad, int ld_out,
                        void* stream);
/* STFT post: spec [M, ld_spec] = [re(0..F-1) | im(0..F-1)] -> mag [M, ld_mag] (zero padded to
 * ld_mag), phase [M, F] (atan2(im, re)) (stft.py:74-79)                                     */
int aldm_mag_phase(const float* spec, float* mag, float* phase, int64_t M, int F, int ld_spec,
                   int ld_mag, void* stream);

/* out[m] = ||x[m, 0:F]||_2 over rows of pitch ld (energy = torch.norm(magnitudes, dim=1),
 * stft.py:176)                                                                              */
int aldm_row_l2norm(const float* x, float* out, int64_t M, int F, int ld, void* stream);

/* ---- CLAP audio tower glue (re-ranking of n_candidate_gen_per_text candidates, ddpm.py:1554-1568) ---------------------- */
/* torchaudio.functional.resample's polyphase windowed-sinc FIR (encoders/modules.py:700-703): y[b, n*up + i] =
 * sum_j xpad[b, n*down + j] * kernel[i, j] with x zero padded by `width` on the left; kernel [up, taps].           */
int aldm_resample_sinc(const float* x, const float* kernel, float* y, int B, int T, int Tout, int down, int up, int taps,
                       int width, void* stream);
/* |STFT|^2 of rows [re | im] (torchlibrosa Spectrogram, power 2: clap/open_clip/htsat.py:889-897), zero padded to ld_out */
int aldm_power_spec(const float* spec, float* out, int64_t M, int F, int ld_spec, int ld_out, void* stream);
/* y[r, c] = x[r, c]*scale[c] + shift[c]: BatchNorm2d over the mel bins in eval mode (htsat.py:1118-1120)             */
int aldm_col_affine(const float* x, const float* scale, const float* shift, float* y, int64_t rows, int C, void* stream);
/* reshape_wav2img (htsat.py:1064-1090: bicubic stretch of T frames to S*S/mel, align_corners, then the fold into an S x S
 * image) fused with the im2col of the 4x4 / stride-4 PatchEmbed conv: x [B, T, mel] -> out [B, (S/p)^2, p*p]         */
int aldm_bicubic_patchify(const float* x, float* out, int B, int T, int mel, int S, int p, void* stream);
/* y[b, c] = mean over the L tokens of x[b, :, c] (HTSAT "embedding", htsat.py:1034-1035)                             */
int aldm_token_mean(const float* x, float* y, int B, int L, int C, void* stream);
/* out[m] = cos(a[m], b[m]) with F.cosine_similarity's eps clamp (encoders/modules.py:651)                            */
int aldm_row_cosine(const float* a, const float* b, float* out, int M, int C, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALDM_HIP_H */
