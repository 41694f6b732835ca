// elementwise.hip — HBM-bound glue kernels of the sampling path: GEGLU gate, timestep embedding,
// layout changes at the UNet boundary, the fused CFG + DDIM update, reflect padding and STFT
// magnitude/phase.  16-byte accesses wherever the layout allows, grid-stride, fp32.
#include "common.h"

namespace aldm {

static inline int ew_blocks(int64_t n, int per_thread = 1) {
    int64_t b = cdiv64(n, 256ll * per_thread);
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// y[m, c] = x[m, c] * gelu(x[m, C + c]);  C % 4 == 0
__global__ void geglu_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t M, int C) {
    const int C4 = C >> 2;
    const int64_t total = M * C4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / C4;
        const int c4 = (int)(i - m * C4);
        const float* xr = x + m * 2 * C;
        const f32x4 a = *reinterpret_cast<const f32x4*>(xr + 4 * c4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(xr + C + 4 * c4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = a[e] * act_apply(g[e], ALDM_ACT_GELU, 0.f);
        *reinterpret_cast<f32x4*>(y + m * C + 4 * c4) = o;
    }
}

// out[b, :half] = cos(t[b]*f_i), out[b, half:2half] = sin(t[b]*f_i), f_i = exp(-ln(P)*i/half)
__global__ void timestep_embedding_kernel(const float* __restrict__ t, float* __restrict__ out, int B,
                                          int dim, float max_period) {
    const int half = dim / 2;
    const int total = B * dim;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / dim, c = i - b * dim;
        float v = 0.f;
        if (c < 2 * half) {
            const int j = c < half ? c : c - half;
            const float freq = expf(-logf(max_period) * (float)j / (float)half);
            const float arg = t[b] * freq;
            v = c < half ? cosf(arg) : sinf(arg);
        }
        out[i] = v;
    }
}

// x [B, C, HW] -> y [rep, B, HW, C]
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C,
                                    int HW, int rep) {
    const int64_t total = (int64_t)B * C * HW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        // i indexes the OUTPUT (coalesced stores): ((b*HW + p)*C + c)
        const int c = (int)(i % C);
        const int64_t bp = i / C;
        const int p = (int)(bp % HW);
        const int b = (int)(bp / HW);
        const float v = x[((int64_t)b * C + c) * HW + p];
        for (int r = 0; r < rep; ++r) y[r * total + i] = v;
    }
}

// x [B, HW, C] -> y [B, C, HW]
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C,
                                    int HW) {
    const int64_t total = (int64_t)B * C * HW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const int64_t bc = i / HW;
        const int c = (int)(bc % C);
        const int b = (int)(bc / C);
        y[i] = x[((int64_t)b * HW + p) * C + c];
    }
}

__global__ void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                 const float* __restrict__ noise, const float* __restrict__ coef,
                                 float* __restrict__ x_prev, float* __restrict__ pred_x0, int64_t n) {
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], c4 = coef[4], gs = coef[5];
    const bool cfg = coef[6] != 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float e;
        if (cfg) {
            const float eu = eps[i], ec = eps[n + i];
            e = eu + gs * (ec - eu);
        } else {
            e = eps[i];
        }
        const float xv = x[i];
        const float p0 = (xv - c0 * e) / c1;
        const float dir = c2 * e;
        const float nz = c4 * noise[i];
        x_prev[i] = c3 * p0 + dir + nz;
        if (pred_x0) pred_x0[i] = p0;
    }
}

// The same update with the step's coefficient row and noise row selected ON THE DEVICE by a step counter, in place on x:
// one captured graph serves every step with no host-issued copies between replays.
__global__ void ddim_step_indexed_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                         const float* __restrict__ noise_tab, const float* __restrict__ coef_tab,
                                         const int* __restrict__ step_idx, float* __restrict__ pred_x0, int64_t n,
                                         int coef_ld) {
    const int s = *step_idx;
    const float* coef = coef_tab + (int64_t)s * coef_ld;
    const float* noise = noise_tab + (int64_t)s * n;
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], c4 = coef[4], gs = coef[5];
    const bool cfg = coef[6] != 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float e;
        if (cfg) {
            const float eu = eps[i], ec = eps[n + i];
            e = eu + gs * (ec - eu);
        } else {
            e = eps[i];
        }
        const float xv = x[i];
        const float p0 = (xv - c0 * e) / c1;
        const float dir = c2 * e;
        const float nz = c4 * noise[i];
        x[i] = c3 * p0 + dir + nz;
        if (pred_x0) pred_x0[i] = p0;
    }
}

// ---- PLMS (pseudo linear multistep, plms.py:261-360): sigma = 0, so no noise operand ------------------------------------------
// the step's model output: the optional CFG combine of eps[2, n], coef[5] / coef[6] as in ddim_step_kernel
__device__ __forceinline__ float plms_model_out(const float* __restrict__ eps, int64_t i, int64_t n, bool cfg, float gs) {
    if (cfg) {
        const float eu = eps[i], ec = eps[n + i];
        return eu + gs * (ec - eu);
    }
    return eps[i];
}

// Step 0 (plms.py:341-345, pseudo improved Euler).  e_next == nullptr: the provisional x_out = update(x, e_t), nothing else
// is written but pred_x0.  Otherwise e' = (e_t + e_next) / 2, x_out = update(x, e'), and e_t opens the history ring (slot 0).
// x_out may be x itself: every element is read before it is written, by the thread that writes it.
__global__ void plms_first_step_kernel(const float* x, const float* __restrict__ e_t, const float* __restrict__ e_next,
                                       const float* __restrict__ coef, float* x_out, float* __restrict__ pred_x0,
                                       float* __restrict__ hist, int64_t n) {
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], gs = coef[5];
    const bool cfg = coef[6] != 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float e = plms_model_out(e_t, i, n, cfg, gs);
        float ep = e;
        if (e_next) {
            ep = (e + plms_model_out(e_next, i, n, cfg, gs)) / 2.0f;
            hist[i] = e;
        }
        const float p0 = (x[i] - c0 * ep) / c1;
        x_out[i] = c3 * p0 + c2 * ep;
        if (pred_x0) pred_x0[i] = p0;
    }
}

// Steps >= 1 with the order, the coefficient row and the ring slots selected ON THE DEVICE by the step counter, in place on x:
// one captured graph serves every step.  The model output of step j lives in ring slot j % 3, so at step s the newest entry
// is slot (s - 1) % 3 and e_t goes where the oldest was, slot s % 3 — no rotation, no pointer swap.  Every thread reads its
// element of all slabs before it writes its one slot.  Sums in the reference's order (plms.py:346-356), then the division.
__global__ void plms_step_indexed_kernel(float* __restrict__ x, const float* __restrict__ eps, float* hist,
                                         const float* __restrict__ coef_tab, const int* __restrict__ step_idx,
                                         float* __restrict__ pred_x0, int64_t n, int coef_ld) {
    const int s = *step_idx;
    if (s < 1) return;   // step 0 has no history: plms_first_step_kernel
    const int k = s < 3 ? s : 3;
    const float* coef = coef_tab + (int64_t)s * coef_ld;
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], gs = coef[5];
    const bool cfg = coef[6] != 0.f;
    const float* h1 = hist + (int64_t)((s + 2) % 3) * n;
    const float* h2 = hist + (int64_t)((s + 1) % 3) * n;
    float* h3 = hist + (int64_t)(s % 3) * n;   // the oldest entry (read only at order 3), then e_t's slot
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float e = plms_model_out(eps, i, n, cfg, gs);
        float ep;
        if (k == 1) {
            ep = (3.0f * e - h1[i]) / 2.0f;
        } else if (k == 2) {
            ep = (23.0f * e - 16.0f * h1[i] + 5.0f * h2[i]) / 12.0f;
        } else {
            ep = (55.0f * e - 59.0f * h1[i] + 37.0f * h2[i] - 9.0f * h3[i]) / 24.0f;
        }
        const float p0 = (x[i] - c0 * ep) / c1;
        x[i] = c3 * p0 + c2 * ep;
        if (pred_x0) pred_x0[i] = p0;
        h3[i] = e;
    }
}

// ---- DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2), deterministic, data-prediction form ----------------------------------------
// Row s = *step_idx of coef_tab = {sigma_t, alpha_t, sigma_prev / sigma_t, -alpha_prev * expm1(-h), w, guidance scale, cfg flag}:
//   x0 = (x - sigma_t e) / alpha_t;  D = x0 (w == 0: a first-order step) or x0 + w (x0 - x0_last);  x = c2 x + c3 D;  x0_last = x0.
struct dpmpp_row {
    float c0, c1, c2, c3, w, gs;
    bool cfg, second;
};

__device__ __forceinline__ dpmpp_row dpmpp_load_row(const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int coef_ld) {
    const float* coef = coef_tab + (int64_t)*step_idx * coef_ld;
    return {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6] != 0.f, coef[4] != 0.f};
}

// one element: x and x0 are updated in place; `old` (the previous step's x0) is read only on a second-order step
__device__ __forceinline__ void dpmpp_elem(const dpmpp_row& r, float& x, float eu, float ec, float old, float& x0) {
    const float e = r.cfg ? eu + r.gs * (ec - eu) : eu;
    const float p0 = (x - r.c0 * e) / r.c1;
    const float d = r.second ? p0 + r.w * (p0 - old) : p0;
    x = r.c2 * x + r.c3 * d;
    x0 = p0;
}

// x0_buf is the one-slab history AND the pred_x0 output: each thread reads its old element, then writes the new x0.  With w == 0
// the old element is not even loaded, so an uninitialised (or NaN) slab cannot reach x.  The counter is trusted as in
// ddim_step_indexed_kernel: step_advance_kernel saturates it at the table's last row.
__global__ void dpmpp_step_indexed_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ x0_buf,
                                          const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int64_t n,
                                          int coef_ld) {
    const dpmpp_row r = dpmpp_load_row(coef_tab, step_idx, coef_ld);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float xv = x[i], p0;
        dpmpp_elem(r, xv, eps[i], r.cfg ? eps[n + i] : 0.f, r.second ? x0_buf[i] : 0.f, p0);
        x[i] = xv;
        x0_buf[i] = p0;
    }
}

// the same with 16 bytes per lane and access: n4 = n / 4 for n % 4 == 0 and 16-byte aligned operands (so is eps + n then)
__global__ void dpmpp_step_indexed_vec4_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ x0_buf,
                                               const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int64_t n4,
                                               int coef_ld) {
    const dpmpp_row r = dpmpp_load_row(coef_tab, step_idx, coef_ld);
    f32x4* xq = reinterpret_cast<f32x4*>(x);
    f32x4* hq = reinterpret_cast<f32x4*>(x0_buf);
    const f32x4* eq = reinterpret_cast<const f32x4*>(eps);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 xv = xq[i], p0;
        const f32x4 eu = eq[i];
        const f32x4 ec = r.cfg ? eq[n4 + i] : zero;
        const f32x4 old = r.second ? hq[i] : zero;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float xk = xv[k], pk;
            dpmpp_elem(r, xk, eu[k], ec[k], old[k], pk);
            xv[k] = xk;
            p0[k] = pk;
        }
        xq[i] = xv;
        hq[i] = p0;
    }
}

// ---- DPM-Solver++(2M) SDE (Lu et al. 2022, the SDE variant in its midpoint form; eta from the ODE solver to the full SDE) -------
// The same row, with c2 = (sigma_prev / sigma_t) exp(-eta h), c3 = -alpha_prev expm1(-(1 + eta) h) and, in column 8,
// c4 = sigma_prev sqrt(-expm1(-2 eta h)):  dpmpp_elem's expression and order, then  x = (c2 x + c3 D) + c4 z,  z the step's unit
// noise: row clamp(*step_idx, 0, noise_rows - 1) of noise_tab [noise_rows, n] — the blend kernels' clamp, so the launch stays inside
// the table whatever the counter holds.  The product c4 z and the sum are rounded separately (no contraction).  With c4 == 0 the noise
// element is not even loaded: a NaN table cannot reach x and the launch is bitwise dpmpp_step_indexed_kernel's.
__device__ __forceinline__ int64_t dpmpp_sde_noise_row(const int* __restrict__ step_idx, int noise_rows) {
    const int s = *step_idx;
    return s < 0 ? 0 : (s > noise_rows - 1 ? noise_rows - 1 : s);
}

__global__ void dpmpp_sde_step_indexed_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ x0_buf,
                                              const float* __restrict__ noise_tab, int noise_rows,
                                              const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int64_t n,
                                              int coef_ld) {
    const dpmpp_row r = dpmpp_load_row(coef_tab, step_idx, coef_ld);
    const float c4 = coef_tab[(int64_t)*step_idx * coef_ld + 8];
    const bool noisy = c4 != 0.f;
    const float* noise = noise_tab + dpmpp_sde_noise_row(step_idx, noise_rows) * n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float xv = x[i], p0;
        dpmpp_elem(r, xv, eps[i], r.cfg ? eps[n + i] : 0.f, r.second ? x0_buf[i] : 0.f, p0);
        if (noisy) {
            const float nz = c4 * noise[i];
            xv = xv + nz;
        }
        x[i] = xv;
        x0_buf[i] = p0;
    }
}

// the same with 16 bytes per lane and access: n4 = n / 4 for n % 4 == 0 and 16-byte aligned operands (so is every noise row then)
__global__ void dpmpp_sde_step_indexed_vec4_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                                   float* __restrict__ x0_buf, const float* __restrict__ noise_tab, int noise_rows,
                                                   const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int64_t n4,
                                                   int coef_ld) {
    const dpmpp_row r = dpmpp_load_row(coef_tab, step_idx, coef_ld);
    const float c4 = coef_tab[(int64_t)*step_idx * coef_ld + 8];
    const bool noisy = c4 != 0.f;
    f32x4* xq = reinterpret_cast<f32x4*>(x);
    f32x4* hq = reinterpret_cast<f32x4*>(x0_buf);
    const f32x4* eq = reinterpret_cast<const f32x4*>(eps);
    const f32x4* nq = reinterpret_cast<const f32x4*>(noise_tab) + dpmpp_sde_noise_row(step_idx, noise_rows) * n4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 xv = xq[i], p0;
        const f32x4 eu = eq[i];
        const f32x4 ec = r.cfg ? eq[n4 + i] : zero;
        const f32x4 old = r.second ? hq[i] : zero;
        const f32x4 nv = noisy ? nq[i] : zero;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float xk = xv[k], pk;
            dpmpp_elem(r, xk, eu[k], ec[k], old[k], pk);
            if (noisy) {
                const float nz = c4 * nv[k];
                xk = xk + nz;
            }
            xv[k] = xk;
            p0[k] = pk;
        }
        xq[i] = xv;
        hq[i] = p0;
    }
}

// ---- guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4) -------------
// Row s = *step_idx (row 0 without a counter) of coef_tab: column 5 = guidance scale, column 7 = phi.  Per sample b of eps[2, B, n_s]:
//   e_g = e_u + s (e_c - e_u);  f = phi std(e_c) / std(e_g) + (1 - phi);  out = f e_g      (f = 1 when std(e_g) == 0 or n_s == 1)
// One workgroup of 1024 threads per sample, three sweeps over the sample's two slabs (the second and third come from L2): the
// means, then the sums of squared deviations from them (two-pass: E[x^2] - E[x]^2 loses the digits the mean takes), then the
// apply.  e_g is the same expression in every sweep.  Each thread accumulates its strided elements in order, a wave reduces by
// shuffles, the 16 wave partials go through LDS and EVERY thread adds them in slot order: a fixed order, no atomics, no flags,
// and one f for the whole workgroup.  A NaN or Inf in a sample reaches its statistics and so all of that sample's outputs.
constexpr int kRescaleThreads = 1024;

// (a, b) summed over the workgroup, the totals returned in every thread; sm: one slot per wave
__device__ __forceinline__ void rescale_block_sum2(float& a, float& b, float (*sm)[2]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6][0] = a;
        sm[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = 0.f;
    b = 0.f;
#pragma unroll
    for (int w = 0; w < kRescaleThreads / 64; ++w) {
        a += sm[w][0];
        b += sm[w][1];
    }
    __syncthreads();   // the slots are free for the next reduction
}

template <int W>
__device__ __forceinline__ void rescale_load(const float* __restrict__ p, float (&v)[W]) {
    if constexpr (W == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q[k];
    } else {
        v[0] = *p;
    }
}

// W floats per lane and access: 4 for n_s % 4 == 0 and 16-byte aligned eps / out (every sample's slabs are aligned then), else 1
template <int W>
__global__ __launch_bounds__(kRescaleThreads) void cfg_rescale_indexed_kernel(const float* __restrict__ eps, float* __restrict__ out,
                                                                              const float* __restrict__ coef_tab,
                                                                              const int* __restrict__ step_idx, int B, int64_t n_s,
                                                                              int coef_ld) {
    __shared__ float sm[kRescaleThreads / 64][2];
    const float* coef = coef_tab + (step_idx ? (int64_t)*step_idx : 0) * coef_ld;
    const float gs = coef[5], phi = coef[7];
    const int64_t b = blockIdx.x;
    const float* eu = eps + b * n_s;
    const float* ec = eps + (B + b) * n_s;
    float* o = out + b * n_s;
    const int64_t nv = n_s / W;
    const float n = (float)n_s;

    // W accumulators per thread and statistic (one per element of an access), added in element order after the sweep
    float pc[W] = {}, pg[W] = {};
    for (int64_t i = threadIdx.x; i < nv; i += kRescaleThreads) {
        float u[W], c[W];
        rescale_load<W>(eu + i * W, u);
        rescale_load<W>(ec + i * W, c);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            pc[k] += c[k];
            pg[k] += u[k] + gs * (c[k] - u[k]);
        }
    }
    float sc = pc[0], sg = pg[0];
#pragma unroll
    for (int k = 1; k < W; ++k) {
        sc += pc[k];
        sg += pg[k];
    }
    rescale_block_sum2(sc, sg, sm);
    const float mc = sc / n, mg = sg / n;

#pragma unroll
    for (int k = 0; k < W; ++k) pc[k] = pg[k] = 0.f;
    for (int64_t i = threadIdx.x; i < nv; i += kRescaleThreads) {
        float u[W], c[W];
        rescale_load<W>(eu + i * W, u);
        rescale_load<W>(ec + i * W, c);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float dc = c[k] - mc;
            const float dg = (u[k] + gs * (c[k] - u[k])) - mg;
            pc[k] += dc * dc;
            pg[k] += dg * dg;
        }
    }
    float qc = pc[0], qg = pg[0];
#pragma unroll
    for (int k = 1; k < W; ++k) {
        qc += pc[k];
        qg += pg[k];
    }
    rescale_block_sum2(qc, qg, sm);
    // std(e_c) / std(e_g): the 1 / n (or 1 / (n - 1)) of both cancels
    const float f = (qg == 0.f || n_s == 1) ? 1.0f : phi * (sqrtf(qc) / sqrtf(qg)) + (1.0f - phi);

    for (int64_t i = threadIdx.x; i < nv; i += kRescaleThreads) {
        float u[W], c[W];
        rescale_load<W>(eu + i * W, u);
        rescale_load<W>(ec + i * W, c);
        if constexpr (W == 4) {
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = f * (u[k] + gs * (c[k] - u[k]));
            *reinterpret_cast<f32x4*>(o + i * 4) = r;
        } else {
            o[i] = f * (u[0] + gs * (c[0] - u[0]));
        }
    }
}

// ---- composable guidance (Liu et al. 2022, "Compositional Visual Generation with Composable Diffusion Models") --------------------
// eps [(K+1), n]: group 0 the unconditional prediction, groups 1..K the prompts'.  Row r = clamp(*step_idx, 0, rows - 1) (row 0
// without a counter) of w_tab [rows, K+1] = {c_0 = 1 - sum w_k, c_1 = w_1, ..., c_K = w_K}, so that
//   e_c = sum_g c_g eps[g]  ==  e_u + sum_k w_k (eps[k] - e_u)
// is the conditional half of the standard pair: the guidance scale multiplies the whole sum where the pair is combined, downstream.
// The row is read once per thread, outside the element loop.  A group whose coefficient is exactly 0 is skipped BEFORE its element is
// loaded (window_merge_rows_kernel's rule: no 0 * NaN, no traffic); the first kept term is a plain multiply, every later one one fma,
// in ascending g; no kept term: 0.  K = 1, w = 1 is {0, 1}: e_c is eps[1] bit for bit.
// pair: out[0:n] = eps[0] bitwise (not rewritten when out == eps) and out[n:2n] = e_c; else out[0:n] = e_c.  out may BE eps: a thread
// owns element i of every group and stores only after it has loaded all of them.  eps and out are therefore not __restrict__.
template <int W>
__global__ void cfg_compose_indexed_kernel(const float* eps, float* out, const float* __restrict__ w_tab,
                                           const int* __restrict__ step_idx, int rows, int K, int pair, int64_t n) {
    int r = step_idx ? *step_idx : 0;
    r = r < 0 ? 0 : (r > rows - 1 ? rows - 1 : r);
    float c[ALDM_MAX_COMPOSE + 1];
#pragma unroll
    for (int g = 0; g <= ALDM_MAX_COMPOSE; ++g) c[g] = g <= K ? w_tab[(int64_t)r * (K + 1) + g] : 0.f;
    const bool copy_u = pair && out != eps;
    float* oc = out + (pair ? n : 0);
    const int64_t nv = n / W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        float acc[W], v[W];
        bool any = false;
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] = 0.f;
#pragma unroll
        for (int g = 0; g <= ALDM_MAX_COMPOSE; ++g) {
            if (c[g] == 0.f) continue;   // uniform over the grid: groups past K have c == 0 too
            rescale_load<W>(eps + (int64_t)g * n + i * W, v);
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] = any ? __builtin_fmaf(c[g], v[k], acc[k]) : c[g] * v[k];
            any = true;
        }
        if (copy_u) {
            rescale_load<W>(eps + i * W, v);
            if constexpr (W == 4) {
                const f32x4 q = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(out + i * 4) = q;
            } else {
                out[i] = v[0];
            }
        }
        if constexpr (W == 4) {
            const f32x4 q = {acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f32x4*>(oc + i * 4) = q;
        } else {
            oc[i] = acc[0];
        }
    }
}

// last node of the step graph: counter += 1 and the NEXT step's timestep row into the UNet's static input (one block: every
// thread reads the old counter before thread 0 stores the new one)
__global__ void step_advance_kernel(int* __restrict__ step_idx, const float* __restrict__ t_tab, float* __restrict__ t_cur,
                                    int nt, int steps) {
    // the counter saturates at the last row: a replay past the end of the run (an extra run_step()) re-reads the last step's
    // coefficient / noise / timestep rows instead of indexing the tables out of bounds
    const int s = *step_idx + 1;
    const int row = s < steps ? s : steps - 1;
    for (int j = threadIdx.x; j < nt; j += blockDim.x) t_cur[j] = t_tab[(int64_t)row * nt + j];
    __syncthreads();
    if (threadIdx.x == 0) *step_idx = row;
}

__global__ void axpby_kernel(const float* __restrict__ a, const float* __restrict__ b,
                             float* __restrict__ y, float alpha, float beta, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float v = alpha * a[i];
        if (b) v += beta * b[i];
        y[i] = v;
    }
}

// y[b, i] = x[b, reflect(i - pad)], i in [0, T + 2*pad)
__global__ void reflect_pad_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T,
                                   int pad, int ld_out) {
    const int To = T + 2 * pad;
    const int64_t total = (int64_t)B * To;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / To);
        int j = (int)(i - (int64_t)b * To) - pad;
        if (j < 0) j = -j;
        if (j >= T) j = 2 * (T - 1) - j;
        y[(int64_t)b * ld_out + (i - (int64_t)b * To)] = x[(int64_t)b * T + j];
    }
}

__global__ void mag_phase_kernel(const float* __restrict__ spec, float* __restrict__ mag,
                                 float* __restrict__ phase, int64_t M, int F, int ld_spec, int ld_mag) {
    const int64_t total = M * ld_mag;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / ld_mag;
        const int f = (int)(i - m * ld_mag);
        float mg = 0.f;
        if (f < F) {
            const float re = spec[m * ld_spec + f], im = spec[m * ld_spec + F + f];
            mg = sqrtf(re * re + im * im);
            if (phase) phase[m * F + f] = atan2f(im, re);
        }
        mag[i] = mg;
    }
}

// out[m] = sqrt(sum_f x[m, f]^2): one wave64 per row (torch.norm(magnitudes, dim=1), stft.py:176)
__global__ __launch_bounds__(256) void row_l2norm_kernel(const float* __restrict__ x,
                                                         float* __restrict__ out, int64_t M, int F,
                                                         int ld) {
    const int lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (row >= M) return;
    float s = 0.f;
    for (int f = lane; f < F; f += 64) {
        const float v = x[row * ld + f];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[row] = sqrtf(s);
}

}  // namespace aldm

using namespace aldm;

extern "C" int aldm_row_l2norm(const float* x, float* out, int64_t M, int F, int ld, void* stream) {
    ALDM_CHECK(x && out && M > 0 && F > 0 && ld >= F, "aldm_row_l2norm: bad args");
    hipLaunchKernelGGL(row_l2norm_kernel, dim3((unsigned)cdiv64(M, 4)), dim3(256), 0,
                       (hipStream_t)stream, x, out, M, F, ld);
    ALDM_LAUNCH_CHECK("aldm_row_l2norm");
    return 0;
}

extern "C" int aldm_geglu(const float* x, float* y, int64_t M, int C, void* stream) {
    ALDM_CHECK(x && y && M > 0 && C > 0 && C % 4 == 0, "aldm_geglu: bad args (C=%d)", C);
    hipLaunchKernelGGL(geglu_kernel, dim3(ew_blocks(M * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       x, y, M, C);
    ALDM_LAUNCH_CHECK("aldm_geglu");
    return 0;
}

extern "C" int aldm_timestep_embedding(const float* t, float* out, int B, int dim, float max_period,
                                       void* stream) {
    ALDM_CHECK(t && out && B > 0 && dim > 0, "aldm_timestep_embedding: bad args");
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(ew_blocks((int64_t)B * dim)), dim3(256), 0,
                       (hipStream_t)stream, t, out, B, dim, max_period);
    ALDM_LAUNCH_CHECK("aldm_timestep_embedding");
    return 0;
}

extern "C" int aldm_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, int rep,
                                 void* stream) {
    ALDM_CHECK(x && y && B > 0 && C > 0 && HW > 0 && rep > 0, "aldm_nchw_to_nhwc: bad args");
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_blocks((int64_t)B * C * HW)), dim3(256), 0,
                       (hipStream_t)stream, x, y, B, C, HW, rep);
    ALDM_LAUNCH_CHECK("aldm_nchw_to_nhwc");
    return 0;
}

extern "C" int aldm_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, void* stream) {
    ALDM_CHECK(x && y && B > 0 && C > 0 && HW > 0, "aldm_nhwc_to_nchw: bad args");
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ew_blocks((int64_t)B * C * HW)), dim3(256), 0,
                       (hipStream_t)stream, x, y, B, C, HW);
    ALDM_LAUNCH_CHECK("aldm_nhwc_to_nchw");
    return 0;
}

extern "C" int aldm_ddim_step(const float* x, const float* eps, const float* noise, const float* coef,
                              float* x_prev, float* pred_x0, int64_t n, void* stream) {
    ALDM_CHECK(x && eps && noise && coef && x_prev && n > 0, "aldm_ddim_step: bad args");
    hipLaunchKernelGGL(ddim_step_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps,
                       noise, coef, x_prev, pred_x0, n);
    ALDM_LAUNCH_CHECK("aldm_ddim_step");
    return 0;
}

extern "C" int aldm_ddim_step_indexed(float* x, const float* eps, const float* noise_tab, const float* coef_tab,
                                      const int* step_idx, float* pred_x0, int64_t n, int coef_ld, void* stream) {
    ALDM_CHECK(x && eps && noise_tab && coef_tab && step_idx && n > 0 && coef_ld >= 7, "aldm_ddim_step_indexed: bad args");
    hipLaunchKernelGGL(ddim_step_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps, noise_tab,
                       coef_tab, step_idx, pred_x0, n, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_ddim_step_indexed");
    return 0;
}

extern "C" int aldm_plms_first_step(const float* x, const float* e_t, const float* e_next, const float* coef_row, float* x_out,
                                    float* pred_x0, float* hist, int64_t n, void* stream) {
    ALDM_CHECK(x && e_t && coef_row && x_out && n > 0 && (!e_next || hist), "aldm_plms_first_step: bad args");
    hipLaunchKernelGGL(plms_first_step_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, e_t, e_next, coef_row,
                       x_out, pred_x0, hist, n);
    ALDM_LAUNCH_CHECK("aldm_plms_first_step");
    return 0;
}

extern "C" int aldm_plms_step_indexed(float* x, const float* eps, float* hist, const float* coef_tab, const int* step_idx,
                                      float* pred_x0, int64_t n, int coef_ld, void* stream) {
    ALDM_CHECK(x && eps && hist && coef_tab && step_idx && n > 0 && coef_ld >= 7, "aldm_plms_step_indexed: bad args");
    hipLaunchKernelGGL(plms_step_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps, hist, coef_tab,
                       step_idx, pred_x0, n, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_plms_step_indexed");
    return 0;
}

extern "C" int aldm_dpmpp_step_indexed(float* x, const float* eps, float* x0_buf, const float* coef_tab, const int* step_idx,
                                       int64_t n, int coef_ld, void* stream) {
    ALDM_CHECK(x && eps && x0_buf && coef_tab && step_idx, "aldm_dpmpp_step_indexed: null pointer");
    ALDM_CHECK(n > 0 && coef_ld >= 7, "aldm_dpmpp_step_indexed: bad args (n=%lld, coef_ld=%d: rows of >= 7 floats)", (long long)n,
               coef_ld);
    const bool vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)x0_buf) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(dpmpp_step_indexed_vec4_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, eps, x0_buf,
                           coef_tab, step_idx, n / 4, coef_ld);
    else
        hipLaunchKernelGGL(dpmpp_step_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps, x0_buf,
                           coef_tab, step_idx, n, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_dpmpp_step_indexed");
    return 0;
}

extern "C" int aldm_dpmpp_sde_step_indexed(float* x, const float* eps, float* x0_buf, const float* noise_tab, int noise_rows,
                                           const float* coef_tab, const int* step_idx, int64_t n, int coef_ld, void* stream) {
    ALDM_CHECK(x && eps && x0_buf && noise_tab && coef_tab && step_idx, "aldm_dpmpp_sde_step_indexed: null pointer");
    ALDM_CHECK(n > 0 && noise_rows >= 1 && coef_ld >= 9,
               "aldm_dpmpp_sde_step_indexed: bad args (n=%lld, noise_rows=%d, coef_ld=%d: rows of >= 9 floats)", (long long)n,
               noise_rows, coef_ld);
    // both in-place operands against the whole table: a step writes them while it reads its noise row
    const uintptr_t t0 = (uintptr_t)noise_tab, t1 = t0 + (uintptr_t)noise_rows * (uintptr_t)n * sizeof(float);
    const uintptr_t nb = (uintptr_t)n * sizeof(float);
    ALDM_CHECK((uintptr_t)x + nb <= t0 || t1 <= (uintptr_t)x, "aldm_dpmpp_sde_step_indexed: x overlaps noise_tab");
    ALDM_CHECK((uintptr_t)x0_buf + nb <= t0 || t1 <= (uintptr_t)x0_buf, "aldm_dpmpp_sde_step_indexed: x0_buf overlaps noise_tab");
    const bool vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)eps | (uintptr_t)x0_buf | (uintptr_t)noise_tab) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(dpmpp_sde_step_indexed_vec4_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, eps,
                           x0_buf, noise_tab, noise_rows, coef_tab, step_idx, n / 4, coef_ld);
    else
        hipLaunchKernelGGL(dpmpp_sde_step_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps, x0_buf,
                           noise_tab, noise_rows, coef_tab, step_idx, n, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_dpmpp_sde_step_indexed");
    return 0;
}

extern "C" int aldm_cfg_rescale_indexed(const float* eps, float* out, const float* coef_tab, const int* step_idx, int B, int64_t n_s,
                                        int coef_ld, void* stream) {
    ALDM_CHECK(eps && out && coef_tab, "aldm_cfg_rescale_indexed: null pointer");
    ALDM_CHECK(B > 0 && B <= 65535 && n_s > 0 && n_s <= (1ll << 40), "aldm_cfg_rescale_indexed: bad args (B=%d, n_s=%lld)", B,
               (long long)n_s);
    ALDM_CHECK(coef_ld >= 8, "aldm_cfg_rescale_indexed: coef_ld=%d: rows of >= 8 floats (column 5 the scale, column 7 phi)", coef_ld);
    const int64_t n = (int64_t)B * n_s;
    ALDM_CHECK(out + n <= eps || eps + 2 * n <= out, "aldm_cfg_rescale_indexed: out overlaps eps");
    const bool vec = n_s % 4 == 0 && (((uintptr_t)eps | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(cfg_rescale_indexed_kernel<4>, dim3((unsigned)B), dim3(kRescaleThreads), 0, (hipStream_t)stream, eps, out,
                           coef_tab, step_idx, B, n_s, coef_ld);
    else
        hipLaunchKernelGGL(cfg_rescale_indexed_kernel<1>, dim3((unsigned)B), dim3(kRescaleThreads), 0, (hipStream_t)stream, eps, out,
                           coef_tab, step_idx, B, n_s, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_cfg_rescale_indexed");
    return 0;
}

extern "C" int aldm_cfg_compose_indexed(const float* eps, float* out, const float* w_tab, const int* step_idx, int rows, int K,
                                        int pair, int64_t n, void* stream) {
    ALDM_CHECK(eps && out && w_tab, "aldm_cfg_compose_indexed: null pointer");
    ALDM_CHECK(K >= 1 && K <= ALDM_MAX_COMPOSE, "aldm_cfg_compose_indexed: K=%d prompts (1 <= K <= %d)", K, ALDM_MAX_COMPOSE);
    ALDM_CHECK(rows >= 1, "aldm_cfg_compose_indexed: rows=%d: the weight table needs at least one row", rows);
    ALDM_CHECK(pair == 0 || pair == 1, "aldm_cfg_compose_indexed: pair=%d must be 0 or 1", pair);
    ALDM_CHECK(n > 0 && n <= (1ll << 40), "aldm_cfg_compose_indexed: bad args (n=%lld)", (long long)n);
    const uintptr_t nb = (uintptr_t)n * sizeof(float);
    const uintptr_t e0 = (uintptr_t)eps, e1 = e0 + (uintptr_t)(K + 1) * nb;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(pair ? 2 : 1) * nb;
    const uintptr_t t0 = (uintptr_t)w_tab, t1 = t0 + (uintptr_t)rows * (uintptr_t)(K + 1) * sizeof(float);
    // in place is the one legal overlap: a thread stores element i only after it has loaded element i of every group
    ALDM_CHECK(o0 == e0 || o1 <= e0 || e1 <= o0, "aldm_cfg_compose_indexed: out overlaps eps (only out == eps, in place, is allowed)");
    ALDM_CHECK(o1 <= t0 || t1 <= o0, "aldm_cfg_compose_indexed: out overlaps w_tab");
    const bool vec = n % 4 == 0 && ((e0 | o0) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(cfg_compose_indexed_kernel<4>, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, eps, out, w_tab,
                           step_idx, rows, K, pair, n);
    else
        hipLaunchKernelGGL(cfg_compose_indexed_kernel<1>, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, eps, out, w_tab,
                           step_idx, rows, K, pair, n);
    ALDM_LAUNCH_CHECK("aldm_cfg_compose_indexed");
    return 0;
}

extern "C" int aldm_step_advance(int* step_idx, const float* t_tab, float* t_cur, int nt, int steps, void* stream) {
    ALDM_CHECK(step_idx && t_tab && t_cur && nt > 0 && steps > 0, "aldm_step_advance: bad args");
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_idx, t_tab, t_cur, nt, steps);
    ALDM_LAUNCH_CHECK("aldm_step_advance");
    return 0;
}

// ancestral DDPM step (ddpm.py:357-373, 1127-1181), same operation order as the reference:
//   x_recon = a*x - b*eps ; mean = c1*x_recon + c2*x ; x_prev = mean + s*noise
// coef = {a = sqrt(1/abar_t), b = sqrt(1/abar_t - 1), c1, c2 (posterior mean), s = nonzero*exp(0.5*logvar)}
__global__ void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                 const float* __restrict__ noise, const float* __restrict__ coef,
                                 float* __restrict__ x_prev, int64_t n) {
    const float a = coef[0], b = coef[1], c1 = coef[2], c2 = coef[3], sg = coef[4];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float xv = x[i];
        const float x0 = a * xv - b * eps[i];
        const float mean = c1 * x0 + c2 * xv;
        x_prev[i] = mean + sg * noise[i];
    }
}

// inpainting blend (ddim.py:226-231 with q_sample ddpm.py:430-436):
//   x = (sa*x0 + so*qnoise)*mask + (1 - mask)*x ;  coef = {sa = sqrt(abar_t), so = sqrt(1 - abar_t)}
__global__ void inpaint_blend_kernel(const float* __restrict__ x0, const float* __restrict__ qnoise,
                                     const float* __restrict__ mask, const float* __restrict__ coef,
                                     float* __restrict__ x, int64_t n) {
    const float sa = coef[0], so = coef[1];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float m = mask[i];
        const float orig = sa * x0[i] + so * qnoise[i];
        x[i] = orig * m + (1.0f - m) * x[i];
    }
}

// the forward jump of resampled inpainting (RePaint, Lugmayr et al. 2022, section 4.2), in place on the whole latent, between two
// replays of the step graph:  x = c0*x + c1*noise_tab[s],  s = *step_idx (row 0 without a counter), {c0, c1} = coef_tab[s][0..1] =
// {sqrt(rho), sqrt(1 - rho)}, rho = abar(k') / abar(k): q(x_k' | x_k) over the whole jump in one launch.  Two rounded products and
// one rounded sum, in that order.  The counter is trusted as in ddim_step_indexed_kernel: step_advance_kernel saturates it at the
// tables' last row.
__global__ void renoise_indexed_kernel(float* __restrict__ x, const float* __restrict__ noise_tab, const float* __restrict__ coef_tab,
                                       const int* __restrict__ step_idx, int64_t n, int coef_ld) {
    const int s = step_idx ? *step_idx : 0;
    const float c0 = coef_tab[(int64_t)s * coef_ld], c1 = coef_tab[(int64_t)s * coef_ld + 1];
    const float* noise = noise_tab + (int64_t)s * n;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float a = c0 * x[i];
        const float b = c1 * noise[i];
        x[i] = a + b;
    }
}

// the same with 16 bytes per lane and access: n4 = n / 4 for n % 4 == 0 and 16-byte aligned x and noise_tab (so is every row then)
__global__ void renoise_indexed_vec4_kernel(float* __restrict__ x, const float* __restrict__ noise_tab,
                                            const float* __restrict__ coef_tab, const int* __restrict__ step_idx, int64_t n4,
                                            int coef_ld) {
    const int s = step_idx ? *step_idx : 0;
    const float c0 = coef_tab[(int64_t)s * coef_ld], c1 = coef_tab[(int64_t)s * coef_ld + 1];
    f32x4* xq = reinterpret_cast<f32x4*>(x);
    const f32x4* nq = reinterpret_cast<const f32x4*>(noise_tab) + (int64_t)s * n4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 xv = xq[i];
        const f32x4 nv = nq[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = c0 * xv[k];
            const float b = c1 * nv[k];
            xv[k] = a + b;
        }
        xq[i] = xv;
    }
}

// graded keep levels (differential diffusion, Levin & Fried 2023), in front of a step's blend:  mask = level > thr_tab[r] ? 1 : 0,
// r = the counter clamped into [0, rows - 1] (row 0 without a counter) — the blend-gather kernels' conventions.  The blend then reads
// a BINARY mask: a frame of level m is held on q_sample(source, t) while the step's threshold lies below m and is free afterwards.
// The comparison is an ordered one, so a NaN level gives 0; the two values stored are the bit patterns of 0.0f and 1.0f.
__device__ __forceinline__ float keep_threshold_row(const float* __restrict__ thr_tab, const int* __restrict__ step_idx, int rows) {
    int r = step_idx ? *step_idx : 0;
    r = r < 0 ? 0 : (r > rows - 1 ? rows - 1 : r);
    return thr_tab[r];
}

__global__ void keep_threshold_indexed_kernel(const float* __restrict__ level, const float* __restrict__ thr_tab,
                                              const int* __restrict__ step_idx, int rows, float* __restrict__ mask, int64_t n) {
    const float thr = keep_threshold_row(thr_tab, step_idx, rows);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = level[i] > thr ? 1.0f : 0.0f;
}

// the same with 16 bytes per lane and access: n4 = n / 4 for n % 4 == 0 and 16-byte aligned level and mask
__global__ void keep_threshold_indexed_vec4_kernel(const float* __restrict__ level, const float* __restrict__ thr_tab,
                                                   const int* __restrict__ step_idx, int rows, float* __restrict__ mask,
                                                   int64_t n4) {
    const float thr = keep_threshold_row(thr_tab, step_idx, rows);
    const f32x4* lq = reinterpret_cast<const f32x4*>(level);
    f32x4* mq = reinterpret_cast<f32x4*>(mask);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 lv = lq[i];
        f32x4 mv;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            mv[k] = lv[k] > thr ? 1.0f : 0.0f;
        mq[i] = mv;
    }
}

// VAE posterior sample fused with the forward diffusion to the sampler's first noise level (audio-to-audio, SDEdit):
//   lv = clamp(logvar, -30, 20); std = exp(0.5 lv); z = scale*(mean + std*n_post); x_t[r] = sa*z[r % B0] + so*n_enc[r]
// coef = {scale, sa = sqrt(abar), so = sqrt(1 - abar)}.  One thread per (source sample, pixel): adjacent threads take adjacent
// pixels, each reads its 2C contiguous channels-last moments as 16-byte words and writes C channel planes (NCHW), every plane
// store coalesced across the wave.  The clamp is two selects, so a NaN logvar stays NaN as under torch.clamp (fminf / fmaxf
// would return the bound).
__global__ void posterior_qsample_kernel(const float* __restrict__ moments_cl, const float* __restrict__ n_post,
                                         const float* __restrict__ n_enc, const float* __restrict__ coef,
                                         float* __restrict__ z, float* __restrict__ x_t, int B0, int n_gen, int C, int64_t hw) {
    const float scale = coef[0], sa = coef[1], so = coef[2];
    const int C4 = C >> 2;
    const int64_t total = (int64_t)B0 * hw;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / hw, p = i - b * hw;
        const float* m = moments_cl + i * 2 * C;
        for (int c4 = 0; c4 < C4; ++c4) {
            const f32x4 mean = *reinterpret_cast<const f32x4*>(m + 4 * c4);
            const f32x4 logvar = *reinterpret_cast<const f32x4*>(m + C + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float lv = logvar[e];
                lv = lv < -30.0f ? -30.0f : lv;
                lv = lv > 20.0f ? 20.0f : lv;
                const float sd = expf(0.5f * lv);
                const int64_t plane = (int64_t)(4 * c4 + e) * hw + p;
                const int64_t j = b * C * hw + plane;
                const float zv = scale * (mean[e] + sd * n_post[j]);
                z[j] = zv;
                const float az = sa * zv;
                for (int g = 0; g < n_gen; ++g) {
                    const int64_t k = ((int64_t)g * B0 + b) * C * hw + plane;   // candidate-major: row r = g*B0 + b reads z[r % B0]
                    x_t[k] = az + so * n_enc[k];
                }
            }
        }
    }
}

extern "C" int aldm_posterior_qsample(const float* moments_cl, const float* n_post, const float* n_enc, const float* coef, float* z,
                                      float* x_t, int B0, int n_gen, int C, int64_t hw, void* stream) {
    ALDM_CHECK(moments_cl && n_post && n_enc && coef && z && x_t, "aldm_posterior_qsample: null pointer");
    ALDM_CHECK(B0 > 0 && n_gen > 0 && hw > 0, "aldm_posterior_qsample: B0=%d, n_gen=%d and hw=%lld must be positive", B0, n_gen,
               (long long)hw);
    ALDM_CHECK(C > 0 && C % 4 == 0, "aldm_posterior_qsample: C=%d must be a positive multiple of 4", C);
    ALDM_CHECK(((uintptr_t)moments_cl & 15) == 0, "aldm_posterior_qsample: moments_cl must be 16-byte aligned");
    hipLaunchKernelGGL(posterior_qsample_kernel, dim3(ew_blocks((int64_t)B0 * hw)), dim3(256), 0, (hipStream_t)stream, moments_cl,
                       n_post, n_enc, coef, z, x_t, B0, n_gen, C, hw);
    ALDM_LAUNCH_CHECK("aldm_posterior_qsample");
    return 0;
}

extern "C" int aldm_ddpm_step(const float* x, const float* eps, const float* noise, const float* coef,
                              float* x_prev, int64_t n, void* stream) {
    ALDM_CHECK(x && eps && noise && coef && x_prev && n > 0, "aldm_ddpm_step: bad args");
    hipLaunchKernelGGL(ddpm_step_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, eps,
                       noise, coef, x_prev, n);
    ALDM_LAUNCH_CHECK("aldm_ddpm_step");
    return 0;
}

extern "C" int aldm_inpaint_blend(const float* x0, const float* qnoise, const float* mask,
                                  const float* coef, float* x, int64_t n, void* stream) {
    ALDM_CHECK(x0 && qnoise && mask && coef && x && n > 0, "aldm_inpaint_blend: bad args");
    hipLaunchKernelGGL(inpaint_blend_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x0,
                       qnoise, mask, coef, x, n);
    ALDM_LAUNCH_CHECK("aldm_inpaint_blend");
    return 0;
}

extern "C" int aldm_renoise_indexed(float* x, const float* noise_tab, const float* coef_tab, const int* step_idx, int64_t n,
                                    int coef_ld, void* stream) {
    ALDM_CHECK(x && noise_tab && coef_tab, "aldm_renoise_indexed: null pointer");
    ALDM_CHECK(n > 0 && coef_ld >= 2, "aldm_renoise_indexed: bad args (n=%lld, coef_ld=%d: rows of >= 2 floats)", (long long)n,
               coef_ld);
    // the table's row count does not cross this ABI: x is checked against the first row here, against the whole table by the
    // host wrapper, which knows the rows
    ALDM_CHECK(x + n <= noise_tab || noise_tab + n <= x, "aldm_renoise_indexed: x overlaps noise_tab");
    const bool vec = n % 4 == 0 && (((uintptr_t)x | (uintptr_t)noise_tab) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(renoise_indexed_vec4_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, noise_tab,
                           coef_tab, step_idx, n / 4, coef_ld);
    else
        hipLaunchKernelGGL(renoise_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, noise_tab, coef_tab,
                           step_idx, n, coef_ld);
    ALDM_LAUNCH_CHECK("aldm_renoise_indexed");
    return 0;
}

extern "C" int aldm_keep_threshold_indexed(const float* level, const float* thr_tab, const int* step_idx, int rows, float* mask,
                                           int64_t n, void* stream) {
    ALDM_CHECK(level && thr_tab && mask, "aldm_keep_threshold_indexed: null pointer");
    ALDM_CHECK(n > 0 && rows > 0, "aldm_keep_threshold_indexed: bad args (n=%lld, rows=%d: both must be positive)", (long long)n,
               rows);
    // in place would destroy the levels, which every later step thresholds again
    ALDM_CHECK(mask + n <= level || level + n <= mask, "aldm_keep_threshold_indexed: mask overlaps level");
    const bool vec = n % 4 == 0 && (((uintptr_t)level | (uintptr_t)mask) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(keep_threshold_indexed_vec4_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, level,
                           thr_tab, step_idx, rows, mask, n / 4);
    else
        hipLaunchKernelGGL(keep_threshold_indexed_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, level, thr_tab,
                           step_idx, rows, mask, n);
    ALDM_LAUNCH_CHECK("aldm_keep_threshold_indexed");
    return 0;
}

extern "C" int aldm_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n,
                          void* stream) {
    ALDM_CHECK(a && y && n > 0, "aldm_axpby: bad args");
    hipLaunchKernelGGL(axpby_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, y,
                       alpha, beta, n);
    ALDM_LAUNCH_CHECK("aldm_axpby");
    return 0;
}

extern "C" int aldm_reflect_pad_1d(const float* x, float* y, int B, int T, int pad, int ld_out,
                                   void* stream) {
    ALDM_CHECK(x && y && B > 0 && T > 1 && pad >= 0 && pad < T && ld_out >= T + 2 * pad,
               "aldm_reflect_pad_1d: bad args");
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(ew_blocks((int64_t)B * (T + 2 * pad))), dim3(256), 0,
                       (hipStream_t)stream, x, y, B, T, pad, ld_out);
    ALDM_LAUNCH_CHECK("aldm_reflect_pad_1d");
    return 0;
}

extern "C" int aldm_mag_phase(const float* spec, float* mag, float* phase, int64_t M, int F,
                              int ld_spec, int ld_mag, void* stream) {
    ALDM_CHECK(spec && mag && M > 0 && F > 0 && ld_spec >= 2 * F && ld_mag >= F,
               "aldm_mag_phase: bad args");
    hipLaunchKernelGGL(mag_phase_kernel, dim3(ew_blocks(M * ld_mag)), dim3(256), 0,
                       (hipStream_t)stream, spec, mag, phase, M, F, ld_spec, ld_mag);
    ALDM_LAUNCH_CHECK("aldm_mag_phase");
    return 0;
}
