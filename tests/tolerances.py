"""Per-mode parity bars of the GPU tests: every bar is <= 5x the error MEASURED for that mode
(profiles/r04_parity_report.txt, profiles/r05_tolerance_calibration.txt), so the assert that passes in the fp32-grade modes
("bf16x6", the default and the bench headline, and "f32") FAILS for a kernel that silently loses one of the six partial products
(~1e-5, tests/test_dma_gpu.py::test_five_product_gemm_fails_the_fp32_grade_bar) — and for "bf16x3", the opt-in mode with 16-bit
operand significands, which keeps its own (looser) bars.

  quantity                                           measured bf16x6 / f32      bar     measured bf16x3   bar
  one contraction vs fp64 (max-norm)                 1.3e-7 .. 8.9e-7           2e-6    2.3e-6 .. 8.1e-6  5e-5
  ... with a fused norm / activation / attention     1.3e-7 .. 2.3e-6           5e-6    3.6e-6 .. 2.0e-5  5e-5
  ... heavy-tailed stress inputs                     1.1e-6 / 7.0e-7 (attn)     5e-6    5.6e-6 / 1.4e-5   5e-5
  the deliberately FIVE-product GEMM (test hook)     7.3e-6 (fails 2e-6, 5e-6)  —       —                 (passes the old 5e-5)
  UNet forward vs real-reference fixture (max-norm)  1.6e-6 .. 2.3e-6           1e-5    1.0e-5 .. 1.7e-5  2e-4
  VAE / HiFi-GAN vs real-reference fixture           2.6e-6 .. 1.1e-5           4e-5    (same kernels)    2e-4
  5-step latent / mel (relative rms)                 2.0e-6..2.2e-6 / 3.1e-6    1e-5 / 1.5e-5   9.8e-6..1.05e-5 / 1.6e-5   1e-4
  200-step latent / mel (relative rms)               9.5e-7 / 2.0e-6            5e-6 / 1e-5     2.7e-6 / 1.0e-5            1e-4

Every entry of the four shipped tuning tables at its real size, on the kernel it names, against an fp64 tap sum evaluated on the GPU
(tests/test_tuned_geometries_gpu.py, profiles/r08_tuned_geometry_errors.txt; whole tensor / worst 32-column block on its own max|ref|),
measured on the kernels whose K loop accumulates in blocks of K = 1024 (acc_close_block, csrc/igemm_epilogue.h); every case passes:

  table (mode)                                    plain epilogue: whole / worst block (bar)         prologue / GEGLU / f16x3 (bar)
  mi355x_igemm.json (f32)                         1.4e-7 .. 1.6e-6 / 2.0e-7 .. 1.8e-6 (2e-6)        1.2e-7 .. 4.0e-6 / 1.8e-7 .. 4.3e-6 (5e-6)
  mi355x_igemm_bf16x6.json (bf16x6, fp32 A)       2.4e-7 .. 1.0e-6 / 3.1e-7 .. 1.2e-6 (2e-6)        1.2e-7 .. 1.4e-6 / 1.7e-7 .. 1.5e-6 (5e-6)
  mi355x_igemm_dma.json (bf16x6, 3-part image)    2.4e-7 .. 9.6e-7 / 2.7e-7 .. 1.0e-6 (2e-6)        4.7e-7 .. 7.7e-7 / 6.8e-7 .. 1.3e-6 (5e-6)
  mi355x_igemm_dma_bf16x3.json (bf16x3, 2-part)   2.0e-6 .. 3.8e-6 / 2.6e-6 .. 3.9e-6 (5e-5)        3.1e-6 .. 4.5e-6 / 6.5e-6 .. 6.6e-6 (5e-5)
  mi355x_igemm_dma_bf16x3.json (f16x3, fp16)      —                                                 1.4e-7 .. 5.5e-7 / 1.7e-7 .. 7.6e-7 (5e-6)
  plain entries with K >= 3072 at split-K 1 ("bf16x6"): DMA table (42) 3.9e-7 .. 7.3e-7 / 4.7e-7 .. 7.6e-7, bf16x6 table (3) 4.3e-7 .. 5.3e-7 /
  5.0e-7 .. 6.7e-7; torch fp32 matmul over the same taps, every K >= 3072 entry: 2.2e-7 .. 8.0e-7 / 2.8e-7 .. 9.8e-7.
  Before the blocked K loop (one fp32 accumulator over the whole contraction) 23 of those entries, K = 3072 .. 11520, measured 2.0e-6 ..
  3.0e-6 / up to 3.4e-6 and failed the 2e-6 bar; the bar stayed and the kernels changed.  The one f32-table entry of that class (K = 3456,
  128x64 tile, fp32 MFMA, single accumulator: the instantiations that keep it are listed in DESIGN.md 5) measures 1.6e-6 / 1.8e-6.

"f16x3" with ONE outlier channel, against fp64, whole tensor / the columns only small channels feed (tests/test_f16x3_outliers_gpu.py,
profiles/r07_f16x3_outlier_errors.txt; the bars are the fp32-grade ones above, "bf16x6" on the same inputs in brackets):

  quantity                                                        measured f16x3 whole / sub-block      (bf16x6)             bar
  LayerNorm -> Linear, gamma / beta channel x 2^8, x 2^12         3.6e-7 .. 2.6e-6 / 2.4e-7 .. 1.2e-6   (<= 2.7e-6 / 1.5e-6)   5e-6
  GroupNorm + SiLU -> conv3x3, same, n up to 32768                4.1e-7 .. 1.5e-6 / 4.4e-7 .. 1.0e-6   (<= 1.6e-6 / 1.6e-6)   5e-6
  Linear / conv3x3 weight row or column x 2^10                    3.1e-7 .. 7.7e-7 / 4.4e-7 .. 6.8e-7   (<= 5.9e-7 / 5.1e-7)   5e-6
  LayerNorm -> GEGLU -> FF-out, gate / value row x 2^4 .. 2^12    3.9e-7 .. 1.9e-6 / 4.4e-7 .. 9.1e-7   (<= 1.1e-6 / 7.6e-7)   5e-6
    ... one gate row x 2^8 under the former (R c + b)^2 bound     1.1e-6 / 3.4e-5 (fails the sub-block assert alone)           5e-6
  LayerNorm -> QKV -> attention -> to_out, W_v / W_k column, row  5.6e-7 .. 5.8e-6 / 5.5e-7 .. 1.4e-6   (<= 7.0e-6 / 2.2e-6)   5e-6 (+ 2^-24 max|score| log2 e with W_k)

The 64-queries-per-wave attention kernels at ragged lengths, against fp64 (tests/test_attention_qt2_gpu.py,
profiles/r11_attention_qt2_errors.txt; the bars are fused_tol's, set before these kernels were measured on their own):

  quantity                                                        measured (typical .. worst)            bar
  fp32-K/V kernels, ragged Lq / Lk, masks: f32 | bf16x6           3.1e-7 .. 6.4e-7 | 2.5e-7 .. 4.5e-7    5e-6
  ... bf16x3                                                      5.8e-6 .. 1.4e-5                       5e-5
  pre-split TAIL self-attention behind its QKV projection         bf16x6 1.0e-6 .. 1.5e-6                5e-6
  ... bf16x3 | f16x3 (LayerNorm-fed)                              1.2e-5 .. 1.4e-5 | 6.6e-7 .. 8.8e-7    5e-5 | 5e-6
  pre-split schedules 1 / 2 at partial query blocks               bf16x6 4.5e-7 / 4.1e-7, bf16x3 7.6e-6 / 8.4e-6   5e-6, 5e-5 (+ _score_tol for 2)

The launch forms of the vocoder's pre-split stage (hifigan.py Generator._stage_dma), against fp64 (tests/test_vocoder_dma_gpu.py,
profiles/r12_vocoder_dma_errors.txt; two samples of 203 rows, 128 / 192 channels, the planner's tile and forced 64- / 128- / 256-row
tiles without and with split-K 3; the bars are gemm_tol's and tail_tol's, set before these launches were measured on their own):

  quantity                                                        measured bf16x6 (typical .. worst)   bar    measured bf16x3      bar
  conv1: dilated conv on the leaky-relu image, leaky-relu epilogue  4.3e-7 .. 5.8e-7                   2e-6   3.0e-6 .. 3.7e-6     5e-5
  conv2 + residual, image of leaky_relu(result)                   3.5e-7 .. 5.6e-7                     2e-6   2.3e-6 .. 2.8e-6     5e-5
  closing launches: alpha = 1/3, out=, accumulate (one / three)   3.6e-7 .. 6.2e-7 / 3.1e-7 .. 4.2e-7  2e-6   2.8e-6 .. 3.0e-6     5e-5
  polyphase transposed conv on a pre-split operand, row remap     3.9e-7 .. 7.9e-7                     2e-6   3.3e-6 .. 3.6e-6     5e-5
  two-stage generator vs the fp64 oracle: stage 0 pre-split       2.3e-6 (f16x3: the same launches)    4e-5   2.4e-5               2e-4
  ... everything register-staged | torch fp32 on the CPU          2.9e-6 | 2.8e-6                      4e-5   2.9e-6 (six products)

Every launch form of GroupNorm, LayerNorm / RMSNorm and the row softmax (csrc/norm.hip), against fp64 (tests/test_norm_forms_gpu.py,
profiles/r13_norm_forms_errors.txt; the form of each GroupNorm case asserted through aldm_groupnorm_plan; GroupNorm figures per
(sample, group), never below the max-norm).  The bars these ops had (1e-5 / 5e-5 / 1e-5 rstd, 5e-6, 2e-6, 1e-5) were more than 5x
the measured figures and are lowered in that file; the older tests of the same ops keep theirs:

  quantity                                                        measured (typical .. worst)            bar
  GroupNorm output, trend / spike inputs: fused | chunked          1.0e-7 .. 1.3e-7 | 1.0e-7 .. 2.6e-7    1e-6
  ... rstd * gamma                                                 1.0e-7 .. 1.4e-7 | 9e-8 .. 2.8e-7      1e-6
  ... channel offsets of 25 .. 1750 (ratios 1e2, 1e3)              2.4e-7 .. 5.8e-7 | 3.2e-7 .. 1.2e-6    5e-6 (rstd 1e-6)
  ... the spike as a thread's FIRST value, pivot = that value      9.8e-6 (G = 1, fused), 4.0e-6 (chunked): rstd as far off.  The pivot is
      (csrc/norm.hip before this table)                            the median of three since: 1.1e-7 / 1.9e-7 at the same positions
  gn_split image, 3-part | 2-part (+ 2^-17)                        3e-8 .. 1.8e-7, large mean .. 5.0e-7 | 2.1e-6 .. 7.0e-6   9e-7, 2e-6 | 8.5e-6, 9.6e-6
  gn_split fp16 image: excess over 2^-20 |v| + 2^-24 / scale       4e-9 .. 1.1e-7 of max|ref| (5.4e-6 with the former pivot)   5e-7
  LayerNorm, C = 4 .. 2048, M = 1 .. 9 | $ALDM_LN_R = 2, 4         8.9e-8 .. 1.8e-7 | 8.5e-8 .. 1.2e-7 (bitwise the default)   6e-7
  ... mean / std = 100 | torch fp32 F.layer_norm on the CPU        2.0e-6 | 3.2e-6                        max(6e-7, 3 x torch's) = 9.5e-6
  RMSNorm, same shapes                                             8.3e-8 .. 1.6e-7                       8e-7
  row softmax, N = 1 .. 15360: plain | masked | biased             1.5e-7 .. 2.2e-7 | 7e-8 .. 2.0e-7 | 1.3e-7 .. 2.2e-7   9e-7

The launch forms the VAE issues (audioldm2_amd/vae.py), one by one, against fp64 (tests/test_vae_forms_gpu.py,
profiles/r14_vae_forms_errors.txt; two samples of 13 x 16 / 65 x 16 / 5 x 64 / 5 x 32 pixels, 128 .. 512 channels; the 3x3 convs on split
operands on the planner's tile, a forced 128x128 tile and a forced halo form; the bars are the existing ones, set before these launches were
measured on their own; typical .. worst):

  quantity                                                        f32 (register-staged)  bf16x6               f16x3                bar    bf16x3              bar
  ResnetBlock gn_split images, 3-part | fp16: excess over model    —                     1.2e-7 .. 1.9e-7     8e-9 .. 1.4e-8       9e-7 | 5e-7   4.5e-6 .. 7.2e-6   8.5e-6
  1x1 nin_shortcut on the raw image                                2.8e-7 .. 5.0e-7       5.6e-7 .. 9.2e-7     (the same launch)    2e-6   5.0e-6 .. 5.6e-6    5e-5
  conv1 / conv2 + skip vs fp64 of the image: planner               —                     2.8e-7 .. 9.2e-7     2.2e-7 .. 9.4e-7     2e-6   3.4e-6 .. 4.8e-6    5e-5
  ... forced 128x128 tile, no split-K | forced halo form           —                     8.1e-7 .. 1.6e-6 | 8.6e-7 .. 1.2e-6   5.4e-7 .. 1.3e-6 | 5.7e-7 .. 7.8e-7   2e-6   3.5e-6 .. 4.7e-6   5e-5
  ... vs fp64 GroupNorm + SiLU + conv (every form)                 2.4e-7 .. 6.8e-7       2.8e-7 .. 1.6e-6     2.2e-7 .. 1.3e-6     5e-6   4.3e-6 .. 5.7e-6    5e-5
  ResnetBlock.run as a whole                                       3.5e-7 .. 6.9e-7       4.5e-7 .. 8.5e-7     4.3e-7 .. 7.9e-7     5e-6   6.4e-6 .. 7.5e-6    5e-5
  fp16 image at n = 2^20 (C = 128, P = 262144; scale 2^3)          —                     —                    2.0e-7 of max|ref|, 4.5e-9 over the model; 1x1 conv from it 2.9e-7   5e-7; 5e-6
  AttnBlock: qkv projection behind gn_split | the prologue         2.4e-7 .. 2.7e-7       5.8e-7 .. 8.0e-7 | 3.4e-7 .. 4.5e-7   6.4e-7 .. 7.2e-7   5e-6   4.7e-6 .. 4.9e-6    5e-5
  ... gemm_nt on slices at pitch 3C | pack_kn + P V                2.3e-7 | 2.5e-7 .. 3.5e-7   2.0e-7 .. 2.6e-7 | 2.8e-7 .. 4.0e-7   (fp32 operands: as bf16x6)   2e-6   (as bf16x6)   5e-5
  ... softmax_rows | out projection + residual | whole block       9e-8 | 9.5e-8 .. 9.9e-8 | 1.2e-7   1.0e-7 .. 1.3e-7 | 1.3e-7 .. 1.9e-7 | 1.7e-7 .. 2.3e-7   (as bf16x6)   9e-7 | 2e-6 | 5e-6   whole 2.2e-6 .. 2.8e-6   5e-5
  gemm_nt / gemm_packed_batched at K = 3104, 3100                  2.5e-7 / 3.3e-7 .. 4.1e-7 in every mode; torch fp32 bmm 5.9e-7 .. 6.3e-7 / 9.7e-7 .. 1.3e-6             5e-6
  Downsample (0, 1, 0, 1) + k3 s2: staged | planner | forced tile  2.1e-7 .. 2.4e-7       1.9e-7 .. 2.5e-7 | 2.5e-7 .. 2.8e-7 | 9.0e-7 .. 9.9e-7   (as bf16x6)   2e-6   4.5e-6 .. 4.8e-6    5e-5
  Upsample nearest x2 + k3 p1: staged | planner | forced tile      3.0e-7 .. 3.5e-7       3.4e-7 .. 3.8e-7 | 4.6e-7 .. 5.4e-7 | 6.8e-7 .. 7.3e-7   (as bf16x6)   2e-6   4.3e-6 .. 4.5e-6    5e-5
  Decoder.conv_out N = 1 (rows 4 bytes apart) | Encoder.conv_out   1.2e-6 .. 1.3e-6 | 2.7e-6 (N = 16), 3.1e-6 (N = 32): one register-staged kernel in every mode            5e-6
  Decoder.conv_in K = 72 / 144 | Encoder.conv_in K = 36            3.2e-7 / 2.7e-7 | 1.5e-7   3.1e-7 / 2.8e-7 | 1.8e-7   (as bf16x6)                                       2e-6
  VAE of ch = 128, (2, 8, 5, 16) latent: decode / encode pre-split 2.5e-6 / 1.6e-6        2.3e-6 / 1.7e-6      2.4e-6 / 1.5e-6      4e-5   3.6e-5 / 1.6e-5     2e-4
  ... register-staged | torch fp32 on the CPU                      (the same)             2.6e-6 / 2.0e-6 | 1.9e-6 / 9.9e-7                4e-5
  the five-product hook on the chain: skip | conv1 vs its image    1.1e-5 | 7.6e-6 (fail 2e-6; six products: 4.8e-7 | 1.0e-6)

The launch forms the UNet issues (audioldm2_amd/unet.py), one by one, against fp64 (tests/test_unet_forms_gpu.py,
profiles/r25_unet_forms_errors.txt; two or three samples of 13 x 16 / 65 x 16 / 12 x 2 / 32 x 2 pixels or 24 / 64 / 208 tokens, 128 .. 640
channels, the decoder's skip concats with the seam inside a group and between groups; the bars are the existing ones, set before these
launches were measured on their own, and ONE new one: timestep_embedding_tol below, for the timestep embedding, which none of the
existing bars fits; every case passes and no kernel was changed; typical .. worst):

  quantity                                                        f32 (register-staged)  bf16x6               f16x3                bar    bf16x3              bar
  ResBlock gn_split images (x ++ skip), 3-part | fp16: excess      —                     1.1e-7 .. 1.9e-7     7e-9 .. 2.6e-8       9e-7 | 5e-7   4.3e-6 .. 6.7e-6   8.5e-6
  1x1 skip on the raw concat image | the register-staged concat    2.9e-7 .. 6.0e-7       5.1e-7 .. 9.9e-7 | 2.5e-7 .. 5.1e-7   (the same launch)   2e-6   4.7e-6 .. 5.9e-6    5e-5
  conv1 + row bias (a column-slice view) vs fp64 of the image      —                     3.0e-7 .. 6.0e-7     2.2e-7 .. 5.2e-7     2e-6   2.5e-6 .. 3.4e-6    5e-5
  ... forced 128x128 tile | forced halo form (W = 16, 4, 2)        —                     5.3e-7 .. 8.4e-7 | 5.1e-7 .. 6.5e-7   3.6e-7 .. 6.0e-7 | 3.9e-7 .. 5.7e-7   2e-6   2.4e-6 .. 3.3e-6   5e-5
  conv2 + skip vs fp64 of the image (every form)                   —                     2.8e-7 .. 9.8e-7     2.4e-7 .. 8.0e-7     2e-6   2.9e-6 .. 4.1e-6    5e-5
  conv1 / conv2 behind the GroupNorm + SiLU prologue (staged)      2.2e-7 .. 5.0e-7       2.1e-7 .. 7.3e-7     (the same launch)    5e-6   (the same launch)   5e-5
  ResBlock.run as a whole                                          3.1e-7 .. 5.5e-7       2.9e-7 .. 8.6e-7     3.6e-7 .. 8.2e-7     5e-6   4.9e-6 .. 6.5e-6    5e-5
  Downsample pad 1 s2 | Upsample: staged | planner | forced tile   2.3e-7 .. 2.6e-7       1.9e-7 .. 3.4e-7 | 2.7e-7 .. 4.1e-7 | 6.6e-7 .. 9.6e-7   (as bf16x6)   2e-6   4.2e-6 .. 5.0e-6    5e-5
  LayerNorm (norm1 / 2 / 3) fp32 output; its image: exact          1.1e-7 .. 1.8e-7       1.1e-7 .. 1.6e-7     1.1e-7 .. 2.0e-7     6e-7   1.1e-7 .. 1.9e-7    6e-7
  qkv / q2 projection vs fp64 of the operand                       3.4e-7 .. 6.6e-7       5.8e-7 .. 9.8e-7     4.9e-7 .. 7.4e-7     2e-6   4.2e-6 .. 5.6e-6    5e-5
  self-attention vs fp64 of its own q, k, v (L = 24, 64, 208)      4.3e-7 .. 8.8e-7       3.5e-7 .. 7.7e-7     2.5e-7 .. 5.8e-7     5e-6   2.1e-6 .. 4.6e-6    5e-5
  cross-attention, masked T5 (21 keys) / AudioMAE (8) | folded     1.4e-7 .. 3.9e-7       1.3e-7 .. 3.1e-7 | 1.2e-7   1.5e-7 .. 3.4e-7 | 1.1e-7   5e-6   5.2e-6 .. 1.7e-5 | 1.2e-7   5e-5
  out1 / out2 + res | K | V projection of the context              7e-8 .. 2.2e-7 | 2.4e-7   1.1e-7 .. 4.8e-7 | 2.0e-7   1.1e-7 .. 4.2e-7 | 2.0e-7   2e-6   7.1e-7 .. 2.8e-6    5e-5
  GEGLU vs fp64 of the operand                                     7.9e-7 .. 1.5e-6       7.1e-7 .. 1.5e-6     5.1e-7 .. 9.1e-7     5e-6   5.1e-6 .. 8.2e-6    5e-5
  ff2 + res | ff2 alone (the residual is 4 .. 6x the product)      6.5e-8 .. 1.1e-7 | 2.1e-7 .. 3.7e-7   7.4e-8 .. 3.1e-7 | 2.8e-7 .. 8.8e-7   7.0e-8 .. 2.5e-7 | 2.4e-7 .. 7.9e-7   2e-6   1.1e-6 .. 1.6e-6 | 4.0e-6 .. 5.5e-6   5e-5
  BasicTransformerBlock.run | SpatialTransformer.run as a whole    2.2e-7 .. 3.3e-7 | 2.8e-7   3.0e-7 .. 5.2e-7 | 5.5e-7   2.2e-7 .. 4.5e-7 | 5.3e-7   5e-6   3.5e-6 .. 5.7e-6 | 5.2e-6   5e-5
  proj_in behind gn_split (eps 1e-6) | proj_out + res              3.0e-7 .. 4.5e-7 | 2.4e-7   5.8e-7 .. 8.9e-7 | 4.5e-7   4.5e-7 .. 7.5e-7 | 4.5e-7   5e-6 | 2e-6   4.9e-6 .. 5.4e-6 | 2.8e-6   5e-5
  timestep_embedding, per row, absolute: t = 500 | 981 | 999        1.5e-5 | 4.4e-5 | 2.8e-5 in every mode; torch fp32 on the CPU: 1.3e-5 | 2.3e-5 | 2.9e-5      2x torch's (timestep_embedding_tol)
  te0 + SiLU | te2 | film_emb | emb_all (N = 1664, 8320) | slices   2.6e-7 | 2.2e-7 | 8.7e-8 | 1.9e-7 | 2.4e-7   2.5e-7 | 1.5e-7 | 1.2e-7 | 2.7e-7 | 3.1e-7 (one register-staged kernel)   5e-6 | 2e-6
  conv_in K = 72 / 144 | out conv N = 8 / 16 behind the prologue   2.8e-7 | 1.4e-6        2.3e-7 | 1.4e-6      (as bf16x6)          2e-6 | 5e-6
  UNET_TINY / UNET_FILM_TINY, (2, C, 12, 8) latent, vs fp64        1.6e-6 / 1.5e-6        1.4e-6 / 1.3e-6      1.5e-6 / 1.2e-6      1e-5   1.4e-5 / 1.6e-5     2e-4
  ... register-staged | torch fp32 on the CPU                      (the same)             1.3e-6 / 1.1e-6 | 1.9e-6 / 2.0e-6                1e-5
  the five-product hook: conv1 + row bias | ff2 alone | ff2 + res  4.8e-6 | 9.8e-6 (fail 2e-6; six products: 5.9e-7 | 9.7e-7) | 1.98e-6 (passes 2e-6: why ff2 is also held alone)
"""
import os


def mode_now():
    from audioldm2_amd import ops
    return ops.MMA_MODE


def fp32_grade(mode=None):
    return (mode or mode_now()) != "bf16x3"


def gemm_tol(mode=None):
    """One contraction against fp64 of the same fp32 inputs (max|err| / max|ref|)."""
    return 2e-6 if fp32_grade(mode) else 5e-5


# Contractions of K >= LONG_K are also put next to torch's own fp32 matmul over the same taps (tests/test_tuned_geometries_gpu.py):
# the yardstick of what fp32 arithmetic itself loses on the case.
LONG_K = 3072


def act_act_long_k_tol():
    """Activation x activation products (ops.gemm_nt / ops.gemm_packed_batched: the VAE mid attention, 8 x [4096 x 4096] . [4096 x
    512]) with K >= LONG_K and operands of non-zero mean, on the fp32 MFMA in every mode.  Measured on an MI355X against fp64: the
    kernel 3.38e-6 whole / 3.61e-6 worst 32-column block, torch's fp32 bmm on the same operands 3.55e-6 / 3.79e-6
    (profiles/r08_tuned_geometry_errors.txt) — fp32 accumulation itself sits above gemm_tol's 2e-6 there.  The bar is at most twice
    the independent fp32 figure (7.1e-6): 5e-6."""
    return 5e-6


def timestep_embedding_tol(torch_fp32_err):
    """ops.timestep_embedding against [cos | sin](t f_i) in fp64, per row (timestep), max |error| absolute.  The argument t f_i is an
    fp32 number of up to ~1e3, so fp32 arithmetic itself is 1e-5 .. 5e-5 from fp64 there and no bar of the table above applies; the
    yardstick is torch's own fp32 evaluation of the same rows (oracle.unet.timestep_embedding on the CPU) against the same fp64
    values.  Measured on an MI355X (profiles/r25_unet_forms_errors.txt), kernel | torch fp32: t = 0: 0 | 0 (cos 0, sin 0: exact),
    t = 1: 4.6e-8 | 4.9e-8, t = 500: 1.5e-5 | 1.3e-5, t = 981: 4.4e-5 | 2.3e-5, t = 999: 2.8e-5 | 2.9e-5.  The bar is twice the
    independent fp32 figure of the row (`torch_fp32_err`: a float or a tensor of them), as act_act_long_k_tol caps its own."""
    return 2.0 * torch_fp32_err


def fused_tol(mode=None):
    """A contraction behind a fused GroupNorm / activation prologue or in front of a transcendental epilogue, vs fp64."""
    return 5e-6 if fp32_grade(mode) else 5e-5


def stress_tol(mode=None):
    return 5e-6 if fp32_grade(mode) else 5e-5


def unet_tol(mode=None):
    return 1e-5 if fp32_grade(mode) else 2e-4


def tail_tol(mode=None):
    """VAE decode / encode, HiFi-GAN against the real reference's fp32 CPU fixture (its own fp32 noise is in the number)."""
    return 4e-5 if fp32_grade(mode) else 2e-4


def latent_tol(steps, mode=None):
    if not fp32_grade(mode):
        return 1e-4
    return 5e-6 if steps >= 100 else 1e-5


def mel_tol(steps, mode=None):
    if not fp32_grade(mode):
        return 1e-4
    return 1e-5 if steps >= 100 else 1.5e-5


def log_err(value, bar, what=""):
    """Calibration aid: with $ALDM_ERR_LOG set, append (test id, measured error, bar) so the bars can be checked against the
    measured errors in one run (profiles/r05_tolerance_calibration.txt)."""
    path = os.environ.get("ALDM_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{mode_now()}\t{value:.3e}\t{bar:.1e}\n")
    return value


class _F64:
    """torch.nn.functional with every floating tensor argument promoted to fp64: the references of the op tests are evaluated in
    double precision, so a bar of 2e-6 measures the KERNEL's error, not ATen's fp32 accumulation order."""

    def __getattr__(self, name):
        import torch
        fn = getattr(torch.nn.functional, name)

        def up(v):
            if torch.is_tensor(v) and v.is_floating_point():
                return v.double()
            if isinstance(v, (list, tuple)) and v and torch.is_tensor(v[0]):
                return type(v)(up(t) for t in v)
            return v

        def call(*a, **k):
            return fn(*[up(v) for v in a], **{kk: up(v) for kk, v in k.items()})
        return call


F64 = _F64()
