// xattn_fold.hip — cross-attention on a short, fixed context (Lk <= 8 keys: the AudioMAE context of the UNet) as ONE launch per
// sublayer.  The context does not change during a sampling run, so K and V are constants of the job and the two C x C projections
// around the attention fold into two per-sample operands (include/aldm_hip.h, "folded cross-attention"):
//     out = softmax_per_head(LayerNorm(h) Mq_b, mask) Mo_b + b_out + h,     Mq_b: C x C/4,  Mo_b: C/4 x C
// — a quarter of the FLOPs of the to_q / to_out projections, and neither the fp32 q nor the attention image ever reaches HBM.
//
// Block = TM (32 | 64) rows of one sample x one slice of the output columns, 4 or 8 waves:
//   1. LayerNorm, one wave per row (the arithmetic of layernorm_kernel, norm.hip), rows -> 3-part bf16 A image in LDS.
//   2. S^T = Mq^T A^T per (32-column score tile, 32-row tile), one tile per wave: the Mq fragments come straight from global memory
//      (each wave streams its own tile: nothing to share through LDS), the A^T fragments from LDS.  Transposed, a lane holds ITS
//      row's scores — head g of the tile in accumulator registers 4g..4g+3, keys 4 (lane >> 5) + 0..3 — so the 8-wide softmax is
//      lane-local plus one exchange with lane ^ 32 (the layout trick of attn.hip).  P -> 3-part bf16 image in LDS.
//   3. O^T = Mo^T P^T per 32-column output tile, + b_out + h, float4 stores from the accumulator layout.
// Blocks that share a row tile (col_splits > 1: few rows per sample, large folded operands) each redo 1 and 2 — that GEMM is tiny
// — and stream only their slice of Mo.  The geometry is decided in xattn_fold_plan() alone; aldm_xattn_fold_plan reports it.
#include "igemm_epilogue.h"
#include <float.h>
#include <stdlib.h>

namespace aldm {

constexpr int XF_PAD = 8;            // bf16 elements of padding per LDS image row: 16-byte fragments of 16 rows on 16 bank slots
constexpr int XF_PIECE = 1024;       // bytes of one (tile, k-step, part) of a folded image: 64 lanes x 16 bytes
constexpr int XF_LDS_MAX = 160 * 1024;

static inline int xf_np(int C) { return ((C >> 2) + 31) & ~31; }

// lo-order products first (attn.hip): (hi, lo) (lo, hi) (mid, mid) (hi, mid) (mid, hi) (hi, hi)
__device__ __forceinline__ f32x16 xf_mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 acc) {
    constexpr int PA_[6] = {0, 2, 1, 0, 1, 0};
    constexpr int PB_[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
    for (int p = 0; p < 6; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA_[p]], b[PB_[p]], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ void xf_load3(const char* p, u32x4 (&dst)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) dst[q] = *reinterpret_cast<const u32x4*>(p + q * XF_PIECE);
}

template <int MAXV, int RT>
__global__ __launch_bounds__(512) void xattn_folded_kernel(const float* __restrict__ h, float* __restrict__ out,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, const char* __restrict__ mq_img,
                                                           const char* __restrict__ mo_img, const float* __restrict__ b_out,
                                                           const float* __restrict__ mask, int L, int C, int Lk, int row_tiles,
                                                           int col_splits) {
    extern __shared__ __attribute__((aligned(16))) char xf_smem[];
    constexpr int TM = 32 * RT;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const int l31 = lane & 31;
    const int lh = lane >> 5;
    const int b = blockIdx.x / row_tiles;
    const int row0 = (blockIdx.x - b * row_tiles) * TM;   // first row of the tile inside sample b
    const int NP = ((C >> 2) + 31) & ~31;
    const int NT = NP >> 5, KS = C >> 4, NS = NP >> 4, CT = C >> 5;
    const int lda = C + XF_PAD, ldp = NP + XF_PAD;        // LDS row pitches, bf16 elements
    char* a_img = xf_smem;                                // [3 parts][TM][lda] bf16
    char* p_img = xf_smem + 6 * TM * lda;                 // [3 parts][TM][ldp] bf16
    const float* hb = h + (int64_t)b * L * C;

    // ---- 1. LayerNorm: rows row0 .. row0 + TM - 1 (clamped to the sample: rows past L are computed, never stored) ----
    {
        constexpr int R = MAXV == 1 ? 8 : 4;   // rows in flight per wave
        const int C4 = C >> 2;
        f32x4 ga[MAXV], be[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c4 = min(lane + 64 * i, C4 - 1);
            ga[i] = *reinterpret_cast<const f32x4*>(gamma + 4 * c4);
            be[i] = *reinterpret_cast<const f32x4*>(beta + 4 * c4);
        }
        for (int t0 = wave * R; t0 < TM; t0 += nw * R) {
            f32x4 v[R][MAXV];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* xr = hb + (int64_t)min(row0 + t0 + r, L - 1) * C;
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int c4 = lane + 64 * i;
                    v[r][i] = c4 < C4 ? *reinterpret_cast<const f32x4*>(xr + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            float mean[R], rstd[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i) s += (v[r][i][0] + v[r][i][1]) + (v[r][i][2] + v[r][i][3]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                mean[r] = s / (float)C;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    if (lane + 64 * i < C4) {
                        const f32x4 dlt = v[r][i] - mean[r];
                        q += (dlt[0] * dlt[0] + dlt[1] * dlt[1]) + (dlt[2] * dlt[2] + dlt[3] * dlt[3]);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
                rstd[r] = 1.0f / sqrtf(q / (float)C + eps);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int i = 0; i < MAXV; ++i) {
                    const int c4 = lane + 64 * i;
                    if (c4 < C4) {
                        const f32x4 o = (v[r][i] - mean[r]) * rstd[r] * ga[i] + be[i];
                        u32x2 part[3];
                        split4(o, part);
#pragma unroll
                        for (int q = 0; q < 3; ++q)
                            *reinterpret_cast<u32x2*>(a_img + ((q * TM + t0 + r) * lda + 4 * c4) * 2) = part[q];
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- 2. scores + softmax: unit u = (score tile nt, row tile rt), one per wave ----
    {
        // this lane's keys: j = 4 lh + e.  dead: a padded key column (weight 0 unconditionally); off: masked (-FLT_MAX)
        bool dead[4], off[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * lh + e;
            dead[e] = j >= Lk;
            off[e] = mask != nullptr && !dead[e] && mask[(int64_t)b * Lk + min(j, Lk - 1)] != 1.0f;
        }
        const char* mq_b = mq_img + (int64_t)b * NT * KS * (3 * XF_PIECE);
        for (int u = wave; u < NT * RT; u += nw) {
            const int nt = u / RT, rt = u - nt * RT;
            if (row0 + 32 * rt >= L) continue;   // the empty half of a 64-row tail tile (wave uniform)
            const char* ap = mq_b + (int64_t)nt * KS * (3 * XF_PIECE) + lane * 16;
            const char* bp = a_img + ((rt * 32 + l31) * lda + 8 * lh) * 2;
            constexpr int PF = 8;   // k-steps of Mq fragments in flight
            u32x4 ring[PF][3];
#pragma unroll
            for (int i = 0; i < PF; ++i) xf_load3(ap + min(i, KS - 1) * (3 * XF_PIECE), ring[i]);
            f32x16 st;
#pragma unroll
            for (int e = 0; e < 16; ++e) st[e] = 0.f;
            // one k-step from ring slot `slot`; refill: the slot's next occupant (k-step ks + PF, clamped: a re-read never used).
            // The main loop has NO per-step condition: a guarded step made hipcc drain the whole ring (vmcnt(0)) every step.
            auto kstep = [&](int ks, u32x4 (&slot)[3], bool refill) {
                bf16x8 a[3], bb[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) a[q] = __builtin_bit_cast(bf16x8, slot[q]);
                if (refill) xf_load3(ap + min(ks + PF, KS - 1) * (3 * XF_PIECE), slot);
#pragma unroll
                for (int q = 0; q < 3; ++q) bb[q] = *reinterpret_cast<const bf16x8*>(bp + q * (TM * lda * 2) + ks * 32);
                st = xf_mma6(a, bb, st);
            };
            const int KSm = KS & ~(PF - 1);
            for (int k0 = 0; k0 < KSm; k0 += PF) {
#pragma unroll
                for (int i = 0; i < PF; ++i) kstep(k0 + i, ring[i], true);
            }
#pragma unroll
            for (int i = 0; i < PF; ++i)
                if (KSm + i < KS) kstep(KSm + i, ring[i], false);   // the last KS % PF steps (wave uniform)
            // lane (row l31, half lh): registers 4g + e = head g of the tile, key 4 lh + e
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float s[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[e] = st[4 * g + e];
                    s[e] = off[e] ? -FLT_MAX : s[e];     // masked_fill_(~(mask == 1), -finfo.max), as attn.hip
                    s[e] = dead[e] ? -INFINITY : s[e];
                }
                float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
                m = fmaxf(m, __shfl_xor(m, 32));         // key 0 is never dead: m is finite
                f32x4 p;
                float sum = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(s[e] - m);
                    p[e] = pe;
                    sum += pe;
                }
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = p[e] * inv;
                u32x2 part[3];
                split4(p, part);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    *reinterpret_cast<u32x2*>(p_img + ((q * TM + rt * 32 + l31) * ldp + nt * 32 + 8 * g + 4 * lh) * 2) = part[q];
            }
        }
    }
    __syncthreads();

    // ---- 3. O^T = Mo^T P^T per 32-column output tile, all RT row tiles of the block per wave; + bias + residual ----
    {
        const int cpb = CT / col_splits;              // output tiles of this block
        const int ct0 = blockIdx.y * cpb + wave;      // this wave's tiles: ct0, ct0 + nw, ...
        const int units = wave < cpb ? (cpb - wave + nw - 1) / nw : 0;
        const int T = units * NS;                     // the wave's (tile, n-step) sequence, streamed through one ring
        const char* mo_b = mo_img + (int64_t)b * CT * NS * (3 * XF_PIECE) + lane * 16;
        auto mo_at = [&](int t) {
            t = min(t, T - 1);
            const int uu = t / NS;
            return mo_b + ((int64_t)(ct0 + uu * nw) * NS + (t - uu * NS)) * (3 * XF_PIECE);
        };
        const char* bp = p_img + (l31 * ldp + 8 * lh) * 2;
        constexpr int PF = 4;
        u32x4 ring[PF][3];
        if (T > 0) {
#pragma unroll
            for (int i = 0; i < PF; ++i) xf_load3(mo_at(i), ring[i]);
        }
        f32x16 acc[RT];
        f32x4 res[RT][4], bias[4];
        int ns = 0, uu = 0;
        for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = t0 + i;
                if (t < T) {   // wave uniform
                    const int ct = ct0 + uu * nw;
                    if (ns == 0) {   // a new tile: clear, and fetch its bias and residual under the products
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) acc[rt][e] = 0.f;
                            const float* hr = hb + (int64_t)min(row0 + rt * 32 + l31, L - 1) * C + ct * 32 + 4 * lh;
#pragma unroll
                            for (int g = 0; g < 4; ++g) res[rt][g] = *reinterpret_cast<const f32x4*>(hr + 8 * g);
                        }
#pragma unroll
                        for (int g = 0; g < 4; ++g) bias[g] = *reinterpret_cast<const f32x4*>(b_out + ct * 32 + 4 * lh + 8 * g);
                    }
                    bf16x8 a[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) a[q] = __builtin_bit_cast(bf16x8, ring[i][q]);
                    xf_load3(mo_at(t + PF), ring[i]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        if (row0 + 32 * rt < L) {
                            bf16x8 bb[3];
#pragma unroll
                            for (int q = 0; q < 3; ++q)
                                bb[q] = *reinterpret_cast<const bf16x8*>(bp + ((q * TM + rt * 32) * ldp) * 2 + ns * 32);
                            acc[rt] = xf_mma6(a, bb, acc[rt]);
                        }
                    }
                    if (++ns == NS) {
                        // lane (row l31, half lh): registers 4g..4g+3 = output columns 32 ct + 8 g + 4 lh + 0..3
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const int row = row0 + rt * 32 + l31;
                            if (row < L) {
                                float* op = out + ((int64_t)b * L + row) * C + ct * 32 + 4 * lh;
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    f32x4 o;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) o[e] = acc[rt][4 * g + e];
                                    o = o + bias[g] + res[rt][g];
                                    *reinterpret_cast<f32x4*>(op + 8 * g) = o;
                                }
                            }
                        }
                        ns = 0;
                        ++uu;
                    }
                }
            }
        }
    }
}

// One thread per 16-byte piece position of one image (its three parts): 8 entries, each a 32-term dot product in fp64, rounded
// once to fp32 and split exactly.  Off the step (once per job), so nothing here is tuned.
__global__ __launch_bounds__(256) void xattn_fold_prepare_kernel(const float* __restrict__ kv, const float* __restrict__ wq,
                                                                 const float* __restrict__ wout, char* __restrict__ mq_img,
                                                                 char* __restrict__ mo_img, int B, int C, int heads, int Lk) {
    const int NP = ((C >> 2) + 31) & ~31;
    const int KS = C >> 4, NS = NP >> 4;
    const int64_t per = (int64_t)(C >> 3) * NP;   // pieces per (sample, image) = C * NP / 8
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * B * per) return;
    const int which = (int)(idx / (B * per));     // 0: Mq, 1: Mo
    const int64_t rem = idx - which * B * per;
    const int b = (int)(rem / per);
    const int piece = (int)(rem - b * per);
    const int lane = piece & 63, tile_step = piece >> 6;
    const int r = lane & 31, u = lane >> 5;
    const float* kvb = kv + (int64_t)b * Lk * 2 * C;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int n, c;
        if (which == 0) {   // [n tile][k step]
            const int nt = tile_step / KS, ks = tile_step - nt * KS;
            n = 32 * nt + r;
            c = 16 * ks + 8 * u + j;
        } else {            // [c tile][n step]
            const int ct = tile_step / NS, ns = tile_step - ct * NS;
            n = 16 * ns + 8 * u + j;
            c = 32 * ct + r;
        }
        const int head = n >> 3, key = n & 7;
        double acc = 0.0;
        if (head < heads && key < Lk) {
            if (which == 0) {
                const float* kp = kvb + (int64_t)key * 2 * C + head * 32;
                for (int d = 0; d < 32; ++d) acc += (double)wq[(int64_t)(head * 32 + d) * C + c] * (double)kp[d];
                acc *= 0.17677669529663688110 * 1.44269504088896340736;   // 32^-1/2 log2(e)
            } else {
                const float* vp = kvb + (int64_t)key * 2 * C + C + head * 32;
                const float* wp = wout + (int64_t)c * C + head * 32;
                for (int d = 0; d < 32; ++d) acc += (double)vp[d] * (double)wp[d];
            }
        }
        x[j] = (float)acc;
    }
    u32x4 part[3];
    split8_to_parts(x, part, 3);
    char* dst = (which == 0 ? mq_img : mo_img) + ((int64_t)b * per * 3 + (int64_t)tile_step * 3 * 64 + lane) * 16;
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(dst + q * XF_PIECE) = part[q];
}

struct XfPlan {
    int ok;   // 0 unsupported, 1 supported, 2 supported and kept by the in-step gate
    int tile_rows, col_splits, waves, blocks, lds_bytes;
};

// Which levels won their in-step A/B (docs/experiments_r1-r6.md §10.8); a level that did not keeps the unfolded path.
static bool xf_level_wins(int C, int L) {
    (void)C;
    (void)L;
    return true;
}

static XfPlan xattn_fold_plan(int B, int L, int C, int heads, int Lk) {
    XfPlan p = {0, 0, 0, 0, 0, 0};
    if (B < 1 || L < 32 || L % 32 != 0 || C < 32 || C % 32 != 0 || heads * 32 != C || Lk < 1 || Lk > 8) return p;
    const int np = xf_np(C), nt = np / 32, ct = C / 32;
    auto lds_of = [&](int tm) { return 6 * tm * (C + XF_PAD) + 6 * tm * (np + XF_PAD); };
    // 64-row tiles where a 32-row tile has fewer score tiles than waves (C <= 256): all four waves get one, and a row tile's
    // folded operands are fetched half as often
    int rt = (nt <= 2 && C <= 256 && L >= 64) ? 2 : 1;
    if (lds_of(32 * rt) > XF_LDS_MAX) rt = 1;
    if (lds_of(32 * rt) > XF_LDS_MAX || C > 768) return p;   // (LayerNorm rows: at most 3 float4 per lane)
    const int tm = 32 * rt;
    const int rb = B * cdiv(L, tm);
    // one round of blocks on the 256 CUs: split the output columns over as many blocks as still fit it
    int cs = 1;
    for (int d = 1; d <= ct; ++d)
        if (ct % d == 0 && (int64_t)rb * d <= 256) cs = d;
    p.ok = xf_level_wins(C, L) ? 2 : 1;
    p.tile_rows = tm;
    p.col_splits = cs;
    p.waves = nt * rt > 4 ? 8 : 4;
    p.blocks = rb * cs;
    p.lds_bytes = lds_of(tm);
    return p;
}

typedef void (*xf_kernel_t)(const float*, float*, const float*, const float*, float, const char*, const char*, const float*,
                            const float*, int, int, int, int, int);

static xf_kernel_t xf_kernel(int maxv, int rt) {   // (64-row tiles exist at C <= 256 only: xattn_fold_plan)
    if (rt == 2) return maxv == 1 ? xattn_folded_kernel<1, 2> : nullptr;
    switch (maxv) {
        case 1: return xattn_folded_kernel<1, 1>;
        case 2: return xattn_folded_kernel<2, 1>;
        case 3: return xattn_folded_kernel<3, 1>;
        default: return nullptr;
    }
}

// the kernels take up to 160 KiB of dynamic LDS: raise every instantiation's limit once (not a stream operation)
static void xf_raise_lds_limits() {
    static const bool done = [] {
        for (int maxv = 1; maxv <= 3; ++maxv)
            for (int rt = 1; rt <= (maxv == 1 ? 2 : 1); ++rt)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(xf_kernel(maxv, rt)),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, XF_LDS_MAX);
        return true;
    }();
    (void)done;
}

}  // namespace aldm

using namespace aldm;

extern "C" int aldm_xattn_fold_plan(int B, int L, int C, int heads, int Lk, int* tile_rows, int* col_splits, int* waves,
                                    int* blocks, int* lds_bytes) {
    const XfPlan p = xattn_fold_plan(B, L, C, heads, Lk);
    if (tile_rows) *tile_rows = p.tile_rows;
    if (col_splits) *col_splits = p.col_splits;
    if (waves) *waves = p.waves;
    if (blocks) *blocks = p.blocks;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return p.ok;
}

extern "C" int64_t aldm_xattn_fold_bytes(int B, int C) {
    if (B < 1 || C < 32 || C % 32 != 0) return 0;
    return (int64_t)B * C * xf_np(C) * 6;   // 3 parts x 2 bytes
}

extern "C" int aldm_xattn_fold_prepare(const float* kv, const float* wq, const float* wout, void* mq_img, void* mo_img, int B,
                                       int C, int heads, int Lk, void* stream) {
    ALDM_CHECK(kv && wq && wout && mq_img && mo_img, "xattn_fold_prepare: null pointer");
    ALDM_CHECK(B >= 1 && C >= 32 && C % 32 == 0 && heads * 32 == C && Lk >= 1 && Lk <= 8,
               "xattn_fold_prepare: unsupported shape B=%d C=%d heads=%d Lk=%d", B, C, heads, Lk);
    xf_raise_lds_limits();
    const int64_t threads = 2 * (int64_t)B * (C >> 3) * xf_np(C);
    hipLaunchKernelGGL(xattn_fold_prepare_kernel, dim3((unsigned)cdiv64(threads, 256)), dim3(256), 0, (hipStream_t)stream, kv,
                       wq, wout, reinterpret_cast<char*>(mq_img), reinterpret_cast<char*>(mo_img), B, C, heads, Lk);
    ALDM_LAUNCH_CHECK("xattn_fold_prepare");
    return 0;
}

extern "C" int aldm_xattn_folded(const float* h, float* out, const float* gamma, const float* beta, float eps,
                                 const void* mq_img, const void* mo_img, const float* b_out, const float* mask, int B, int L,
                                 int C, int heads, int Lk, void* stream) {
    ALDM_CHECK(h && out && gamma && beta && mq_img && mo_img && b_out, "xattn_folded: null pointer");
    ALDM_CHECK(h != out, "xattn_folded: out must not alias h (the residual is re-read after other blocks have stored)");
    const XfPlan p = xattn_fold_plan(B, L, C, heads, Lk);
    ALDM_CHECK(p.ok != 0, "xattn_folded: unsupported shape B=%d L=%d C=%d heads=%d Lk=%d", B, L, C, heads, Lk);
    xf_raise_lds_limits();
    const xf_kernel_t k = xf_kernel(cdiv(C, 256), p.tile_rows / 32);
    ALDM_CHECK(k != nullptr, "xattn_folded: no kernel for C=%d", C);
    const int row_tiles = cdiv(L, p.tile_rows);
    hipLaunchKernelGGL(k, dim3(B * row_tiles, p.col_splits), dim3(64 * p.waves), p.lds_bytes, (hipStream_t)stream, h, out, gamma,
                       beta, eps, reinterpret_cast<const char*>(mq_img), reinterpret_cast<const char*>(mo_img), b_out, mask, L,
                       C, Lk, row_tiles, p.col_splits);
    ALDM_LAUNCH_CHECK("xattn_folded");
    return 0;
}
