// windows.hip — the per-step launches of windowed (long-form) diffusion: the window gather in front of the UNet pass and the
// tapered, normalised overlap-add behind it, and the gather fused with the inpainting blend of a kept source on
// the long latent (§9f), the wrap-around forms of the three for ring plans (§9g), and their forms over the rows of a prompt timeline
// (one row per window and prompt, the merge weighted per row and frame; §9h).  All are HBM-bound copies with at most `cover` multiply-adds (the blend: five operations) per
// element: 16-byte accesses along the contiguous F axis where F % 4 == 0 and the pointers are aligned, a scalar path otherwise,
// grid-stride, 64-bit indexing, fp32.  The window starts travel as a kernel argument (aldm_window_starts, by value): a captured
// step graph carries them, there is no device table and no copy inside a capture; every index into them is wave-uniform.  The one
// device table is the phase table of the `_ring_phased` forms (moving window phases, §9k): one int32 per visit, read with the step
// counter the graph already advances — a static buffer of the graph, refilled per job outside any capture.
#include "common.h"

namespace aldm {

static inline int win_blocks(int64_t n) {
    int64_t b = cdiv64(n, 256);
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

template <int V> struct vec_of;
template <> struct vec_of<4> { typedef f32x4 type; };
template <> struct vec_of<1> { typedef float type; };

// win[(j*B + b), c, p, f] = x[b, c, s_j + p, f].  blockIdx.y = j; per (b, c) the Tw*F floats are contiguous on both sides.
// per_row = Tw*F / V units per (b, c); total = B*C*per_row units per window.
template <int V>
__global__ void window_gather_kernel(const float* __restrict__ x, float* __restrict__ win, aldm_window_starts st, int T, int F,
                                     int64_t per_row, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int j = blockIdx.y;
    const int64_t src0 = (int64_t)st.s[j] * F;          // the window's offset inside a (b, c) plane of x
    const int64_t plane = (int64_t)T * F;
    float* dst = win + (int64_t)j * total * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = i / per_row, off = i - bc * per_row;
        *reinterpret_cast<vec*>(dst + i * V) = *reinterpret_cast<const vec*>(x + bc * plane + src0 + off * V);
    }
}

// out[h, b, c, t, f] = sum over the windows j that cover t, ascending j, of wn[j, t - s_j] * win[h, j*B + b, c, t - s_j, f]: the
// first term a plain multiply, every later one a fused multiply-add.  Gather form: one thread owns an output element (V of them
// along F), so there are no atomics and the result does not depend on the launch geometry.  total = H*B*C*T*(F/V) units.
template <int V>
__global__ void window_merge_kernel(const float* __restrict__ win, const float* __restrict__ wn, float* __restrict__ out,
                                    aldm_window_starts st, int B, int W, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        q /= C;
        const int b = (int)(q % B);
        const int64_t h = q / B;
        vec acc = vec(0.0f);
        bool first = true;
        for (int j = 0; j < W; ++j) {
            const int p = t - st.s[j];
            if (p < 0 || p >= Tw) continue;
            const float wv = wn[(int64_t)j * Tw + p];
            const vec e = *reinterpret_cast<const vec*>(win + ((((h * W + j) * B + b) * C + c) * wplane + (int64_t)p * F + fv * V));
            if (first) {
                acc = wv * e;
                first = false;
            } else if constexpr (V == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(wv, e[k], acc[k]);
            } else {
                acc = __builtin_fmaf(wv, e, acc);
            }
        }
        *reinterpret_cast<vec*>(out + i * V) = acc;
    }
}

// The inpainting blend on the long latent and the window gather in one launch, scatter form (the mirror image of the merge): one
// thread owns a long-latent element (V of them along F), reads x, x0, qnoise and mask once, writes the blended x back and then every
// window copy of it — at most `cover` of them: win[(j*B + b), c, t - s_j, f] for the windows j with 0 <= t - s_j < Tw.  A window
// position maps to one frame, so every element of win has exactly one writer, and the starts tile [0, T), so every element is
// written: no atomics, independent of the launch geometry.  In place on x: the owner is its element's only reader and writer.  The
// expression and its operation order are inpaint_blend_kernel's (elementwise.hip); built with -ffp-contract=off the launch is
// bitwise that kernel followed by window_gather_kernel.  The q-noise and coefficient rows are selected by the device-side step
// counter, each saturating at its table's last row (q_rows == 1: one staged draw per step).  total = B*C*T*(F/V) units.
template <int V>
__global__ void window_blend_gather_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ qnoise,
                                           const float* __restrict__ mask, const float* __restrict__ blend_coef,
                                           const int* __restrict__ step_idx, int q_rows, int coef_rows, float* __restrict__ win,
                                           aldm_window_starts st, int B, int W, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    int s = step_idx ? *step_idx : 0;
    s = s < 0 ? 0 : s;
    const int qr = s < q_rows ? s : q_rows - 1, cr = s < coef_rows ? s : coef_rows - 1;
    const float sa = blend_coef[2 * cr], so = blend_coef[2 * cr + 1];
    const float* qn = qnoise + (int64_t)qr * total * V;
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        const int64_t b = q / C;
        const vec m = *reinterpret_cast<const vec*>(mask + i * V);
        const vec orig = sa * *reinterpret_cast<const vec*>(x0 + i * V) + so * *reinterpret_cast<const vec*>(qn + i * V);
        const vec v = orig * m + (1.0f - m) * *reinterpret_cast<const vec*>(x + i * V);
        *reinterpret_cast<vec*>(x + i * V) = v;
        for (int j = 0; j < W; ++j) {
            const int p = t - st.s[j];
            if (p < 0 || p >= Tw) continue;
            *reinterpret_cast<vec*>(win + (((int64_t)j * B + b) * C + c) * wplane + (int64_t)p * F + fv * V) = v;
        }
    }
}

// ---- ring plans (seamless loops): the T frames are a circle, window j covers the frames (s_j + p) mod T ------------
// Siblings of the three kernels above rather than a template flag on them: the linear kernels stay, instruction for instruction,
// what they were.  The wrap is along T, so a 16-byte access along F never straddles it; it is a compare and a subtract (add), never
// an integer modulo: 0 <= s_j < T and 0 <= p < Tw <= T bound s_j + p below 2T, and t - s_j above -T.

// win[(j*B + b), c, p, f] = x[b, c, (s_j + p) mod T, f].  A window's Tw*F floats per (b, c) come from at most two contiguous spans
// of x: frames [s_j, min(s_j + Tw, T)) and [0, s_j + Tw - T).  len1 = the first span in units; the span is picked by comparing the
// in-row offset with it (wave-uniform but for the one wave that holds the junction): no division beyond the linear kernel's.
template <int V>
__global__ void window_gather_ring_kernel(const float* __restrict__ x, float* __restrict__ win, aldm_window_starts st, int T, int Tw,
                                          int F, int64_t per_row, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int j = blockIdx.y;
    const int s = st.s[j];
    const int64_t src0 = (int64_t)s * F;
    const int64_t plane = (int64_t)T * F;
    const int64_t len1 = (int64_t)(Tw < T - s ? Tw : T - s) * F / V;
    float* dst = win + (int64_t)j * total * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = i / per_row, off = i - bc * per_row;
        const int64_t src = off < len1 ? src0 + off * V : (off - len1) * V;
        *reinterpret_cast<vec*>(dst + i * V) = *reinterpret_cast<const vec*>(x + bc * plane + src);
    }
}

// window_merge_kernel on a ring: the windows j in ascending order with p = t - s_j (+ T if negative) < Tw.  Tw <= T: a window
// covers a frame at most once.
template <int V>
__global__ void window_merge_ring_kernel(const float* __restrict__ win, const float* __restrict__ wn, float* __restrict__ out,
                                         aldm_window_starts st, int B, int W, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        q /= C;
        const int b = (int)(q % B);
        const int64_t h = q / B;
        vec acc = vec(0.0f);
        bool first = true;
        for (int j = 0; j < W; ++j) {
            int p = t - st.s[j];
            if (p < 0) p += T;
            if (p >= Tw) continue;
            const float wv = wn[(int64_t)j * Tw + p];
            const vec e = *reinterpret_cast<const vec*>(win + ((((h * W + j) * B + b) * C + c) * wplane + (int64_t)p * F + fv * V));
            if (first) {
                acc = wv * e;
                first = false;
            } else if constexpr (V == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(wv, e[k], acc[k]);
            } else {
                acc = __builtin_fmaf(wv, e, acc);
            }
        }
        *reinterpret_cast<vec*>(out + i * V) = acc;
    }
}

// window_blend_gather_kernel on a ring: the same blend expression, operation order and row selection, then every window copy of
// the owned element at its wrapped position.  A window position still maps to one frame, so every element of win has exactly one
// writer, and the windows cover the circle, so every element is written.
template <int V>
__global__ void window_blend_gather_ring_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ qnoise,
                                                const float* __restrict__ mask, const float* __restrict__ blend_coef,
                                                const int* __restrict__ step_idx, int q_rows, int coef_rows,
                                                float* __restrict__ win, aldm_window_starts st, int B, int W, int C, int T, int Tw,
                                                int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    int s = step_idx ? *step_idx : 0;
    s = s < 0 ? 0 : s;
    const int qr = s < q_rows ? s : q_rows - 1, cr = s < coef_rows ? s : coef_rows - 1;
    const float sa = blend_coef[2 * cr], so = blend_coef[2 * cr + 1];
    const float* qn = qnoise + (int64_t)qr * total * V;
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        const int64_t b = q / C;
        const vec m = *reinterpret_cast<const vec*>(mask + i * V);
        const vec orig = sa * *reinterpret_cast<const vec*>(x0 + i * V) + so * *reinterpret_cast<const vec*>(qn + i * V);
        const vec v = orig * m + (1.0f - m) * *reinterpret_cast<const vec*>(x + i * V);
        *reinterpret_cast<vec*>(x + i * V) = v;
        for (int j = 0; j < W; ++j) {
            int p = t - st.s[j];
            if (p < 0) p += T;
            if (p >= Tw) continue;
            *reinterpret_cast<vec*>(win + (((int64_t)j * B + b) * C + c) * wplane + (int64_t)p * F + fv * V) = v;
        }
    }
}

// ---- moving window phases: a ring plan whose starts are all rotated by a phase the step counter selects -------------
// Siblings of the three ring kernels; those stay what they were.  A rigid rotation keeps every gap, so the plan's weights hold for
// every phase.  The phase is chosen ON THE DEVICE: row r = clamp(*step_idx, 0, rows - 1) of the int32 table (step_idx NULL: row 0),
// phi = clamp(phase_tab[r], 0, T - 1) — out-of-range values clamp, they do not wrap: whatever the table holds the launch stays in
// its buffers.  Window j then covers the frames (s_j + phi + p) mod T.  phi is wave-uniform and read once per thread, outside the
// element loop; s_j + phi < 2T, so the rotated start is a compare and a subtract and the kernels below go on as their ring siblings.
__device__ __forceinline__ int window_phase(const int* __restrict__ phase_tab, const int* __restrict__ step_idx, int rows, int T) {
    int r = step_idx ? *step_idx : 0;
    r = r < 0 ? 0 : r;
    r = r < rows ? r : rows - 1;
    int phi = phase_tab[r];
    phi = phi < 0 ? 0 : phi;
    return phi < T ? phi : T - 1;
}

__device__ __forceinline__ int phased_start(int s, int phi, int T) {
    const int e = s + phi;
    return e >= T ? e - T : e;
}

// win[(j*B + b), c, p, f] = x[b, c, (s_j + phi + p) mod T, f]: window_gather_ring_kernel from the rotated start.
template <int V>
__global__ void window_gather_ring_phased_kernel(const float* __restrict__ x, float* __restrict__ win, aldm_window_starts st,
                                                 const int* __restrict__ phase_tab, const int* __restrict__ step_idx, int rows, int T,
                                                 int Tw, int F, int64_t per_row, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int j = blockIdx.y;
    const int s = phased_start(st.s[j], window_phase(phase_tab, step_idx, rows, T), T);
    const int64_t src0 = (int64_t)s * F;
    const int64_t plane = (int64_t)T * F;
    const int64_t len1 = (int64_t)(Tw < T - s ? Tw : T - s) * F / V;
    float* dst = win + (int64_t)j * total * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = i / per_row, off = i - bc * per_row;
        const int64_t src = off < len1 ? src0 + off * V : (off - len1) * V;
        *reinterpret_cast<vec*>(dst + i * V) = *reinterpret_cast<const vec*>(x + bc * plane + src);
    }
}

// window_merge_ring_kernel with rotated starts: the windows j in ascending order with p = t - (s_j + phi) mod T (+ T if negative)
// < Tw — the ring merge's result rolled by +phi along T, term for term.
template <int V>
__global__ void window_merge_ring_phased_kernel(const float* __restrict__ win, const float* __restrict__ wn, float* __restrict__ out,
                                                aldm_window_starts st, const int* __restrict__ phase_tab,
                                                const int* __restrict__ step_idx, int rows, int B, int W, int C, int T, int Tw, int F,
                                                int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int phi = window_phase(phase_tab, step_idx, rows, T);
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        q /= C;
        const int b = (int)(q % B);
        const int64_t h = q / B;
        vec acc = vec(0.0f);
        bool first = true;
        for (int j = 0; j < W; ++j) {
            int p = t - phased_start(st.s[j], phi, T);
            if (p < 0) p += T;
            if (p >= Tw) continue;
            const float wv = wn[(int64_t)j * Tw + p];
            const vec e = *reinterpret_cast<const vec*>(win + ((((h * W + j) * B + b) * C + c) * wplane + (int64_t)p * F + fv * V));
            if (first) {
                acc = wv * e;
                first = false;
            } else if constexpr (V == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(wv, e[k], acc[k]);
            } else {
                acc = __builtin_fmaf(wv, e, acc);
            }
        }
        *reinterpret_cast<vec*>(out + i * V) = acc;
    }
}

// window_blend_gather_ring_kernel with rotated starts: the blend is the sibling's (it does not depend on phi), then every window
// copy of the owned element at its rotated, wrapped position.  A window position still maps to one frame and the rotated windows
// still cover the circle: one writer per element of win, all written.
template <int V>
__global__ void window_blend_gather_ring_phased_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                                       const float* __restrict__ qnoise, const float* __restrict__ mask,
                                                       const float* __restrict__ blend_coef, const int* __restrict__ step_idx,
                                                       int q_rows, int coef_rows, float* __restrict__ win, aldm_window_starts st,
                                                       const int* __restrict__ phase_tab, int rows, int B, int W, int C, int T, int Tw,
                                                       int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    int s = step_idx ? *step_idx : 0;
    s = s < 0 ? 0 : s;
    const int qr = s < q_rows ? s : q_rows - 1, cr = s < coef_rows ? s : coef_rows - 1;
    const float sa = blend_coef[2 * cr], so = blend_coef[2 * cr + 1];
    const float* qn = qnoise + (int64_t)qr * total * V;
    const int phi = window_phase(phase_tab, step_idx, rows, T);
    const int FV = F / V;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        const int64_t b = q / C;
        const vec m = *reinterpret_cast<const vec*>(mask + i * V);
        const vec orig = sa * *reinterpret_cast<const vec*>(x0 + i * V) + so * *reinterpret_cast<const vec*>(qn + i * V);
        const vec v = orig * m + (1.0f - m) * *reinterpret_cast<const vec*>(x + i * V);
        *reinterpret_cast<vec*>(x + i * V) = v;
        for (int j = 0; j < W; ++j) {
            int p = t - phased_start(st.s[j], phi, T);
            if (p < 0) p += T;
            if (p >= Tw) continue;
            *reinterpret_cast<vec*>(win + (((int64_t)j * B + b) * C + c) * wplane + (int64_t)p * F + fv * V) = v;
        }
    }
}

// the host-side checks the ring entries share: the shape, and starts whose windows of Tw cover the circle of T frames
static int window_ring_args_ok(const char* name, const aldm_window_starts& st, int B, int W, int C, int T, int Tw, int F) {
    ALDM_CHECK(B > 0 && C > 0 && F > 0 && Tw > 0 && T >= Tw, "%s: bad shape (B=%d, C=%d, T=%d, Tw=%d, F=%d)", name, B, C, T, Tw, F);
    ALDM_CHECK(W >= 2 && W <= ALDM_MAX_WINDOWS && st.n == W, "%s: W=%d windows with %d starts (2 <= W == n <= %d: a ring of one "
               "window has no window across its junction)", name, W, st.n, ALDM_MAX_WINDOWS);
    ALDM_CHECK(st.s[0] == 0, "%s: starts[0]=%d must be 0", name, st.s[0]);
    for (int j = 1; j < W; ++j) {
        ALDM_CHECK(st.s[j] > st.s[j - 1], "%s: starts must ascend (starts[%d]=%d after %d)", name, j, st.s[j], st.s[j - 1]);
        ALDM_CHECK(st.s[j] < T, "%s: starts[%d]=%d must lie below T=%d", name, j, st.s[j], T);
        ALDM_CHECK(st.s[j] - st.s[j - 1] <= Tw, "%s: gap of %d frames between starts[%d] and starts[%d] exceeds Tw=%d: frames "
                   "without a window", name, st.s[j] - st.s[j - 1], j - 1, j, Tw);
    }
    ALDM_CHECK(T - st.s[W - 1] <= Tw, "%s: gap of %d frames between starts[%d] and the wrap to frame 0 exceeds Tw=%d: frames "
               "without a window", name, T - st.s[W - 1], W - 1, Tw);
    ALDM_CHECK((int64_t)W * B * C * Tw * F <= (1ll << 40), "%s: %lld window elements", name, (long long)W * B * C * Tw * F);
    return 0;
}

// the host-side checks the entries share: the shape, and starts that tile [0, T) with windows of Tw
static int window_args_ok(const char* name, const aldm_window_starts& st, int B, int W, int C, int T, int Tw, int F) {
    ALDM_CHECK(B > 0 && C > 0 && F > 0 && Tw > 0 && T >= Tw, "%s: bad shape (B=%d, C=%d, T=%d, Tw=%d, F=%d)", name, B, C, T, Tw, F);
    ALDM_CHECK(W >= 1 && W <= ALDM_MAX_WINDOWS && st.n == W, "%s: W=%d windows with %d starts (1 <= W == n <= %d)", name, W, st.n,
               ALDM_MAX_WINDOWS);
    ALDM_CHECK(st.s[0] == 0, "%s: starts[0]=%d must be 0", name, st.s[0]);
    for (int j = 1; j < W; ++j) {
        ALDM_CHECK(st.s[j] > st.s[j - 1], "%s: starts must ascend (starts[%d]=%d after %d)", name, j, st.s[j], st.s[j - 1]);
        ALDM_CHECK(st.s[j] - st.s[j - 1] <= Tw, "%s: gap of %d frames between starts[%d] and starts[%d] exceeds Tw=%d: frames "
                   "without a window", name, st.s[j] - st.s[j - 1], j - 1, j, Tw);
    }
    ALDM_CHECK(st.s[W - 1] == T - Tw, "%s: the last start %d must be T - Tw = %d", name, st.s[W - 1], T - Tw);
    ALDM_CHECK((int64_t)W * B * C * Tw * F <= (1ll << 40), "%s: %lld window elements", name, (long long)W * B * C * Tw * F);
    return 0;
}

static inline bool spans_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

// ---- prompt timelines: a ROW is one window under one prompt, so rows may share a start ------------------------------
// Siblings again: the linear and ring kernels above stay what they were.  The row starts travel by value (aldm_window_rows, 64
// entries, 260 bytes of kernel arguments); every index into them is wave-uniform.

// win[(r*B + b), c, p, f] = x[b, c, s_r + p, f].  blockIdx.y = r: window_gather_kernel over rows (rows of one window are equal
// copies; each is read from x again — the long latent is R/W-th of the traffic and stays in L2).
template <int V>
__global__ void window_gather_rows_kernel(const float* __restrict__ x, float* __restrict__ win, aldm_window_rows st, int T, int F,
                                          int64_t per_row, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int r = blockIdx.y;
    const int64_t src0 = (int64_t)st.s[r] * F;
    const int64_t plane = (int64_t)T * F;
    float* dst = win + (int64_t)r * total * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = i / per_row, off = i - bc * per_row;
        *reinterpret_cast<vec*>(dst + i * V) = *reinterpret_cast<const vec*>(x + bc * plane + src0 + off * V);
    }
}

// out[h, b, c, t, f] = sum over the rows r that cover t with wr[r, t - s_r] != 0, ascending r, of wr[r, t - s_r] * win[h, r*B + b, c,
// t - s_r, f]: the first kept term a plain multiply, every later one a fused multiply-add.  A row whose weight at the frame is exactly
// 0 is skipped BEFORE its win element is loaded: a prompt that is silent there contributes nothing (no 0 * NaN) and costs no
// traffic.  The weight depends on (r, t) only: the skip is uniform over the F lanes of an output row.  Gather form, no atomics.
template <int V>
__global__ void window_merge_rows_kernel(const float* __restrict__ win, const float* __restrict__ wr, float* __restrict__ out,
                                         aldm_window_rows st, int B, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int FV = F / V;
    const int R = st.n;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        q /= C;
        const int b = (int)(q % B);
        const int64_t h = q / B;
        vec acc = vec(0.0f);
        bool first = true;
        for (int r = 0; r < R; ++r) {
            const int p = t - st.s[r];
            if (p < 0 || p >= Tw) continue;
            const float wv = wr[(int64_t)r * Tw + p];
            if (wv == 0.0f) continue;
            const vec e = *reinterpret_cast<const vec*>(win + ((((h * R + r) * B + b) * C + c) * wplane + (int64_t)p * F + fv * V));
            if (first) {
                acc = wv * e;
                first = false;
            } else if constexpr (V == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(wv, e[k], acc[k]);
            } else {
                acc = __builtin_fmaf(wv, e, acc);
            }
        }
        *reinterpret_cast<vec*>(out + i * V) = acc;
    }
}

// window_blend_gather_kernel over rows: the same blend expression, operation order and row selection of the tables, then a copy
// into every covering row.  A row position maps to one frame, so every element of win has exactly one writer, and the row starts
// tile [0, T), so every element is written.
template <int V>
__global__ void window_blend_gather_rows_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ qnoise,
                                                const float* __restrict__ mask, const float* __restrict__ blend_coef,
                                                const int* __restrict__ step_idx, int q_rows, int coef_rows,
                                                float* __restrict__ win, aldm_window_rows st, int B, int C, int T, int Tw, int F,
                                                int64_t total) {
    typedef typename vec_of<V>::type vec;
    int s = step_idx ? *step_idx : 0;
    s = s < 0 ? 0 : s;
    const int qr = s < q_rows ? s : q_rows - 1, cr = s < coef_rows ? s : coef_rows - 1;
    const float sa = blend_coef[2 * cr], so = blend_coef[2 * cr + 1];
    const float* qn = qnoise + (int64_t)qr * total * V;
    const int FV = F / V;
    const int R = st.n;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t q = i / FV;
        const int fv = (int)(i - q * FV);
        const int t = (int)(q % T);
        q /= T;
        const int c = (int)(q % C);
        const int64_t b = q / C;
        const vec m = *reinterpret_cast<const vec*>(mask + i * V);
        const vec orig = sa * *reinterpret_cast<const vec*>(x0 + i * V) + so * *reinterpret_cast<const vec*>(qn + i * V);
        const vec v = orig * m + (1.0f - m) * *reinterpret_cast<const vec*>(x + i * V);
        *reinterpret_cast<vec*>(x + i * V) = v;
        for (int r = 0; r < R; ++r) {
            const int p = t - st.s[r];
            if (p < 0 || p >= Tw) continue;
            *reinterpret_cast<vec*>(win + (((int64_t)r * B + b) * C + c) * wplane + (int64_t)p * F + fv * V) = v;
        }
    }
}

// the host-side checks the row entries share: the shape, and row starts (non-decreasing: a window under several prompts repeats its
// start) whose windows of Tw tile [0, T)
static int window_rows_args_ok(const char* name, const aldm_window_rows& st, int B, int C, int T, int Tw, int F) {
    ALDM_CHECK(B > 0 && C > 0 && F > 0 && Tw > 0 && T >= Tw, "%s: bad shape (B=%d, C=%d, T=%d, Tw=%d, F=%d)", name, B, C, T, Tw, F);
    ALDM_CHECK(st.n >= 1 && st.n <= ALDM_MAX_ROWS, "%s: %d rows (1 <= n <= %d)", name, st.n, ALDM_MAX_ROWS);
    ALDM_CHECK(st.s[0] == 0, "%s: rows[0]=%d must be 0", name, st.s[0]);
    for (int r = 1; r < st.n; ++r) {
        ALDM_CHECK(st.s[r] >= st.s[r - 1], "%s: row starts must not decrease (rows[%d]=%d after %d)", name, r, st.s[r], st.s[r - 1]);
        ALDM_CHECK(st.s[r] - st.s[r - 1] <= Tw, "%s: gap of %d frames between rows[%d] and rows[%d] exceeds Tw=%d: frames without "
                   "a row", name, st.s[r] - st.s[r - 1], r - 1, r, Tw);
    }
    ALDM_CHECK(st.s[st.n - 1] == T - Tw, "%s: the last row start %d must be T - Tw = %d", name, st.s[st.n - 1], T - Tw);
    ALDM_CHECK((int64_t)st.n * B * C * Tw * F <= (1ll << 40), "%s: %lld row elements", name, (long long)st.n * B * C * Tw * F);
    return 0;
}

}  // namespace aldm

using namespace aldm;

extern "C" int aldm_window_gather(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F,
                                  void* stream) {
    ALDM_CHECK(x && win, "aldm_window_gather: null pointer");
    if (window_args_ok("aldm_window_gather", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(x, n_x, win, n_w), "aldm_window_gather: win overlaps x");
    const int64_t per_window = (int64_t)B * C * Tw * F;
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)x | (uintptr_t)win) & 15) == 0) {
        const dim3 grid(win_blocks(per_window / 4), W);
        hipLaunchKernelGGL(window_gather_kernel<4>, grid, block, 0, (hipStream_t)stream, x, win, starts, T, F,
                           (int64_t)Tw * F / 4, per_window / 4);
    } else {
        const dim3 grid(win_blocks(per_window), W);
        hipLaunchKernelGGL(window_gather_kernel<1>, grid, block, 0, (hipStream_t)stream, x, win, starts, T, F, (int64_t)Tw * F,
                           per_window);
    }
    ALDM_LAUNCH_CHECK("aldm_window_gather");
    return 0;
}

extern "C" int aldm_window_blend_gather(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                                        const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_starts starts, int B,
                                        int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && x0 && qnoise && mask && blend_coef && win, "aldm_window_blend_gather: null pointer");
    if (window_args_ok("aldm_window_blend_gather", starts, B, W, C, T, Tw, F) != 0) return -1;
    ALDM_CHECK(q_rows >= 1 && coef_rows >= 1, "aldm_window_blend_gather: q_rows=%d and coef_rows=%d must be >= 1", q_rows, coef_rows);
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F, n_q = (int64_t)q_rows * n_x;
    ALDM_CHECK(!spans_overlap(win, n_w, x, n_x) && !spans_overlap(win, n_w, x0, n_x) && !spans_overlap(win, n_w, qnoise, n_q) &&
               !spans_overlap(win, n_w, mask, n_x), "aldm_window_blend_gather: win overlaps x, x0, qnoise or mask");
    ALDM_CHECK(!spans_overlap(x, n_x, x0, n_x) && !spans_overlap(x, n_x, qnoise, n_q) && !spans_overlap(x, n_x, mask, n_x),
               "aldm_window_blend_gather: x overlaps x0, qnoise or mask");
    const dim3 block(256);
    if (F % 4 == 0 &&
        (((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)qnoise | (uintptr_t)mask | (uintptr_t)win) & 15) == 0) {
        hipLaunchKernelGGL(window_blend_gather_kernel<4>, dim3(win_blocks(n_x / 4)), block, 0, (hipStream_t)stream, x, x0, qnoise,
                           mask, blend_coef, step_idx, q_rows, coef_rows, win, starts, B, W, C, T, Tw, F, n_x / 4);
    } else {
        hipLaunchKernelGGL(window_blend_gather_kernel<1>, dim3(win_blocks(n_x)), block, 0, (hipStream_t)stream, x, x0, qnoise, mask,
                           blend_coef, step_idx, q_rows, coef_rows, win, starts, B, W, C, T, Tw, F, n_x);
    }
    ALDM_LAUNCH_CHECK("aldm_window_blend_gather");
    return 0;
}

extern "C" int aldm_window_merge(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W, int C,
                                 int T, int Tw, int F, void* stream) {
    ALDM_CHECK(win && wn && out, "aldm_window_merge: null pointer");
    ALDM_CHECK(H == 1 || H == 2, "aldm_window_merge: H=%d: 1, or 2 for the [uncond ; cond] pair", H);
    if (window_args_ok("aldm_window_merge", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_out = (int64_t)H * B * C * T * F, n_w = (int64_t)H * W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(out, n_out, win, n_w) && !spans_overlap(out, n_out, wn, (int64_t)W * Tw),
               "aldm_window_merge: out overlaps win or wn");
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)win | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(window_merge_kernel<4>, dim3(win_blocks(n_out / 4)), block, 0, (hipStream_t)stream, win, wn, out, starts, B,
                           W, C, T, Tw, F, n_out / 4);
    } else {
        hipLaunchKernelGGL(window_merge_kernel<1>, dim3(win_blocks(n_out)), block, 0, (hipStream_t)stream, win, wn, out, starts, B, W,
                           C, T, Tw, F, n_out);
    }
    ALDM_LAUNCH_CHECK("aldm_window_merge");
    return 0;
}

// ---- the ring entries (ABI v20): the argument lists of their linear siblings ------------------------------------------------------
extern "C" int aldm_window_gather_ring(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw,
                                       int F, void* stream) {
    ALDM_CHECK(x && win, "aldm_window_gather_ring: null pointer");
    if (window_ring_args_ok("aldm_window_gather_ring", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(x, n_x, win, n_w), "aldm_window_gather_ring: win overlaps x");
    const int64_t per_window = (int64_t)B * C * Tw * F;
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)x | (uintptr_t)win) & 15) == 0) {
        const dim3 grid(win_blocks(per_window / 4), W);
        hipLaunchKernelGGL(window_gather_ring_kernel<4>, grid, block, 0, (hipStream_t)stream, x, win, starts, T, Tw, F,
                           (int64_t)Tw * F / 4, per_window / 4);
    } else {
        const dim3 grid(win_blocks(per_window), W);
        hipLaunchKernelGGL(window_gather_ring_kernel<1>, grid, block, 0, (hipStream_t)stream, x, win, starts, T, Tw, F,
                           (int64_t)Tw * F, per_window);
    }
    ALDM_LAUNCH_CHECK("aldm_window_gather_ring");
    return 0;
}

extern "C" int aldm_window_blend_gather_ring(float* x, const float* x0, const float* qnoise, const float* mask,
                                             const float* blend_coef, const int* step_idx, int q_rows, int coef_rows, float* win,
                                             aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && x0 && qnoise && mask && blend_coef && win, "aldm_window_blend_gather_ring: null pointer");
    if (window_ring_args_ok("aldm_window_blend_gather_ring", starts, B, W, C, T, Tw, F) != 0) return -1;
    ALDM_CHECK(q_rows >= 1 && coef_rows >= 1, "aldm_window_blend_gather_ring: q_rows=%d and coef_rows=%d must be >= 1", q_rows,
               coef_rows);
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F, n_q = (int64_t)q_rows * n_x;
    ALDM_CHECK(!spans_overlap(win, n_w, x, n_x) && !spans_overlap(win, n_w, x0, n_x) && !spans_overlap(win, n_w, qnoise, n_q) &&
               !spans_overlap(win, n_w, mask, n_x), "aldm_window_blend_gather_ring: win overlaps x, x0, qnoise or mask");
    ALDM_CHECK(!spans_overlap(x, n_x, x0, n_x) && !spans_overlap(x, n_x, qnoise, n_q) && !spans_overlap(x, n_x, mask, n_x),
               "aldm_window_blend_gather_ring: x overlaps x0, qnoise or mask");
    const dim3 block(256);
    if (F % 4 == 0 &&
        (((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)qnoise | (uintptr_t)mask | (uintptr_t)win) & 15) == 0) {
        hipLaunchKernelGGL(window_blend_gather_ring_kernel<4>, dim3(win_blocks(n_x / 4)), block, 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, starts, B, W, C, T, Tw, F, n_x / 4);
    } else {
        hipLaunchKernelGGL(window_blend_gather_ring_kernel<1>, dim3(win_blocks(n_x)), block, 0, (hipStream_t)stream, x, x0, qnoise,
                           mask, blend_coef, step_idx, q_rows, coef_rows, win, starts, B, W, C, T, Tw, F, n_x);
    }
    ALDM_LAUNCH_CHECK("aldm_window_blend_gather_ring");
    return 0;
}

extern "C" int aldm_window_merge_ring(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W,
                                      int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(win && wn && out, "aldm_window_merge_ring: null pointer");
    ALDM_CHECK(H == 1 || H == 2, "aldm_window_merge_ring: H=%d: 1, or 2 for the [uncond ; cond] pair", H);
    if (window_ring_args_ok("aldm_window_merge_ring", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_out = (int64_t)H * B * C * T * F, n_w = (int64_t)H * W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(out, n_out, win, n_w) && !spans_overlap(out, n_out, wn, (int64_t)W * Tw),
               "aldm_window_merge_ring: out overlaps win or wn");
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)win | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(window_merge_ring_kernel<4>, dim3(win_blocks(n_out / 4)), block, 0, (hipStream_t)stream, win, wn, out,
                           starts, B, W, C, T, Tw, F, n_out / 4);
    } else {
        hipLaunchKernelGGL(window_merge_ring_kernel<1>, dim3(win_blocks(n_out)), block, 0, (hipStream_t)stream, win, wn, out, starts,
                           B, W, C, T, Tw, F, n_out);
    }
    ALDM_LAUNCH_CHECK("aldm_window_merge_ring");
    return 0;
}

// ---- the phased ring entries (ABI v25, moving window phases): the ring entries' checks, plus the phase table ----------------------
// the table is `rows` int32: it may share no byte with a buffer the launch writes
static inline bool phase_tab_overlaps(const int* tab, int rows, const float* buf, int64_t n) {
    return spans_overlap(reinterpret_cast<const float*>(tab), rows, buf, n);
}

extern "C" int aldm_window_gather_ring_phased(const float* x, float* win, aldm_window_starts starts, const int* phase_tab,
                                              const int* step_idx, int rows, int B, int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && win, "aldm_window_gather_ring_phased: null pointer");
    ALDM_CHECK(phase_tab, "aldm_window_gather_ring_phased: null phase table");
    ALDM_CHECK(rows >= 1, "aldm_window_gather_ring_phased: rows=%d must be >= 1", rows);
    if (window_ring_args_ok("aldm_window_gather_ring_phased", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(x, n_x, win, n_w), "aldm_window_gather_ring_phased: win overlaps x");
    ALDM_CHECK(!phase_tab_overlaps(phase_tab, rows, win, n_w), "aldm_window_gather_ring_phased: win overlaps phase_tab");
    const int64_t per_window = (int64_t)B * C * Tw * F;
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)x | (uintptr_t)win) & 15) == 0) {
        const dim3 grid(win_blocks(per_window / 4), W);
        hipLaunchKernelGGL(window_gather_ring_phased_kernel<4>, grid, block, 0, (hipStream_t)stream, x, win, starts, phase_tab,
                           step_idx, rows, T, Tw, F, (int64_t)Tw * F / 4, per_window / 4);
    } else {
        const dim3 grid(win_blocks(per_window), W);
        hipLaunchKernelGGL(window_gather_ring_phased_kernel<1>, grid, block, 0, (hipStream_t)stream, x, win, starts, phase_tab,
                           step_idx, rows, T, Tw, F, (int64_t)Tw * F, per_window);
    }
    ALDM_LAUNCH_CHECK("aldm_window_gather_ring_phased");
    return 0;
}

extern "C" int aldm_window_blend_gather_ring_phased(float* x, const float* x0, const float* qnoise, const float* mask,
                                                    const float* blend_coef, const int* step_idx, int q_rows, int coef_rows,
                                                    float* win, aldm_window_starts starts, const int* phase_tab, int rows, int B,
                                                    int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && x0 && qnoise && mask && blend_coef && win, "aldm_window_blend_gather_ring_phased: null pointer");
    ALDM_CHECK(phase_tab, "aldm_window_blend_gather_ring_phased: null phase table");
    ALDM_CHECK(rows >= 1, "aldm_window_blend_gather_ring_phased: rows=%d must be >= 1", rows);
    if (window_ring_args_ok("aldm_window_blend_gather_ring_phased", starts, B, W, C, T, Tw, F) != 0) return -1;
    ALDM_CHECK(q_rows >= 1 && coef_rows >= 1, "aldm_window_blend_gather_ring_phased: q_rows=%d and coef_rows=%d must be >= 1", q_rows,
               coef_rows);
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F, n_q = (int64_t)q_rows * n_x;
    ALDM_CHECK(!spans_overlap(win, n_w, x, n_x) && !spans_overlap(win, n_w, x0, n_x) && !spans_overlap(win, n_w, qnoise, n_q) &&
               !spans_overlap(win, n_w, mask, n_x), "aldm_window_blend_gather_ring_phased: win overlaps x, x0, qnoise or mask");
    ALDM_CHECK(!spans_overlap(x, n_x, x0, n_x) && !spans_overlap(x, n_x, qnoise, n_q) && !spans_overlap(x, n_x, mask, n_x),
               "aldm_window_blend_gather_ring_phased: x overlaps x0, qnoise or mask");
    ALDM_CHECK(!phase_tab_overlaps(phase_tab, rows, win, n_w) && !phase_tab_overlaps(phase_tab, rows, x, n_x),
               "aldm_window_blend_gather_ring_phased: win or x overlaps phase_tab");
    const dim3 block(256);
    if (F % 4 == 0 &&
        (((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)qnoise | (uintptr_t)mask | (uintptr_t)win) & 15) == 0) {
        hipLaunchKernelGGL(window_blend_gather_ring_phased_kernel<4>, dim3(win_blocks(n_x / 4)), block, 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, starts, phase_tab, rows, B, W, C, T, Tw, F,
                           n_x / 4);
    } else {
        hipLaunchKernelGGL(window_blend_gather_ring_phased_kernel<1>, dim3(win_blocks(n_x)), block, 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, starts, phase_tab, rows, B, W, C, T, Tw, F,
                           n_x);
    }
    ALDM_LAUNCH_CHECK("aldm_window_blend_gather_ring_phased");
    return 0;
}

extern "C" int aldm_window_merge_ring_phased(const float* win, const float* wn, float* out, aldm_window_starts starts,
                                             const int* phase_tab, const int* step_idx, int rows, int H, int B, int W, int C, int T,
                                             int Tw, int F, void* stream) {
    ALDM_CHECK(win && wn && out, "aldm_window_merge_ring_phased: null pointer");
    ALDM_CHECK(phase_tab, "aldm_window_merge_ring_phased: null phase table");
    ALDM_CHECK(rows >= 1, "aldm_window_merge_ring_phased: rows=%d must be >= 1", rows);
    ALDM_CHECK(H == 1 || H == 2, "aldm_window_merge_ring_phased: H=%d: 1, or 2 for the [uncond ; cond] pair", H);
    if (window_ring_args_ok("aldm_window_merge_ring_phased", starts, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_out = (int64_t)H * B * C * T * F, n_w = (int64_t)H * W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(out, n_out, win, n_w) && !spans_overlap(out, n_out, wn, (int64_t)W * Tw),
               "aldm_window_merge_ring_phased: out overlaps win or wn");
    ALDM_CHECK(!phase_tab_overlaps(phase_tab, rows, out, n_out), "aldm_window_merge_ring_phased: out overlaps phase_tab");
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)win | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(window_merge_ring_phased_kernel<4>, dim3(win_blocks(n_out / 4)), block, 0, (hipStream_t)stream, win, wn, out,
                           starts, phase_tab, step_idx, rows, B, W, C, T, Tw, F, n_out / 4);
    } else {
        hipLaunchKernelGGL(window_merge_ring_phased_kernel<1>, dim3(win_blocks(n_out)), block, 0, (hipStream_t)stream, win, wn, out,
                           starts, phase_tab, step_idx, rows, B, W, C, T, Tw, F, n_out);
    }
    ALDM_LAUNCH_CHECK("aldm_window_merge_ring_phased");
    return 0;
}

// ---- the row entries (ABI v22, prompt timelines): rows = (window, prompt) pairs, starts non-decreasing --------------------------------
extern "C" int aldm_window_gather_rows(const float* x, float* win, aldm_window_rows rows, int B, int C, int T, int Tw, int F,
                                       void* stream) {
    ALDM_CHECK(x && win, "aldm_window_gather_rows: null pointer");
    if (window_rows_args_ok("aldm_window_gather_rows", rows, B, C, T, Tw, F) != 0) return -1;
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)rows.n * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(x, n_x, win, n_w), "aldm_window_gather_rows: win overlaps x");
    const int64_t per_window = (int64_t)B * C * Tw * F;
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)x | (uintptr_t)win) & 15) == 0) {
        const dim3 grid(win_blocks(per_window / 4), rows.n);
        hipLaunchKernelGGL(window_gather_rows_kernel<4>, grid, block, 0, (hipStream_t)stream, x, win, rows, T, F,
                           (int64_t)Tw * F / 4, per_window / 4);
    } else {
        const dim3 grid(win_blocks(per_window), rows.n);
        hipLaunchKernelGGL(window_gather_rows_kernel<1>, grid, block, 0, (hipStream_t)stream, x, win, rows, T, F, (int64_t)Tw * F,
                           per_window);
    }
    ALDM_LAUNCH_CHECK("aldm_window_gather_rows");
    return 0;
}

extern "C" int aldm_window_blend_gather_rows(float* x, const float* x0, const float* qnoise, const float* mask,
                                             const float* blend_coef, const int* step_idx, int q_rows, int coef_rows, float* win,
                                             aldm_window_rows rows, int B, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && x0 && qnoise && mask && blend_coef && win, "aldm_window_blend_gather_rows: null pointer");
    if (window_rows_args_ok("aldm_window_blend_gather_rows", rows, B, C, T, Tw, F) != 0) return -1;
    ALDM_CHECK(q_rows >= 1 && coef_rows >= 1, "aldm_window_blend_gather_rows: q_rows=%d and coef_rows=%d must be >= 1", q_rows,
               coef_rows);
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)rows.n * B * C * Tw * F, n_q = (int64_t)q_rows * n_x;
    ALDM_CHECK(!spans_overlap(win, n_w, x, n_x) && !spans_overlap(win, n_w, x0, n_x) && !spans_overlap(win, n_w, qnoise, n_q) &&
               !spans_overlap(win, n_w, mask, n_x), "aldm_window_blend_gather_rows: win overlaps x, x0, qnoise or mask");
    ALDM_CHECK(!spans_overlap(x, n_x, x0, n_x) && !spans_overlap(x, n_x, qnoise, n_q) && !spans_overlap(x, n_x, mask, n_x),
               "aldm_window_blend_gather_rows: x overlaps x0, qnoise or mask");
    const dim3 block(256);
    if (F % 4 == 0 &&
        (((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)qnoise | (uintptr_t)mask | (uintptr_t)win) & 15) == 0) {
        hipLaunchKernelGGL(window_blend_gather_rows_kernel<4>, dim3(win_blocks(n_x / 4)), block, 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, rows, B, C, T, Tw, F, n_x / 4);
    } else {
        hipLaunchKernelGGL(window_blend_gather_rows_kernel<1>, dim3(win_blocks(n_x)), block, 0, (hipStream_t)stream, x, x0, qnoise,
                           mask, blend_coef, step_idx, q_rows, coef_rows, win, rows, B, C, T, Tw, F, n_x);
    }
    ALDM_LAUNCH_CHECK("aldm_window_blend_gather_rows");
    return 0;
}

extern "C" int aldm_window_merge_rows(const float* win, const float* wr, float* out, aldm_window_rows rows, int H, int B, int C, int T,
                                      int Tw, int F, void* stream) {
    ALDM_CHECK(win && wr && out, "aldm_window_merge_rows: null pointer");
    ALDM_CHECK(H == 1 || H == 2, "aldm_window_merge_rows: H=%d: 1, or 2 for the [uncond ; cond] pair", H);
    if (window_rows_args_ok("aldm_window_merge_rows", rows, B, C, T, Tw, F) != 0) return -1;
    const int64_t n_out = (int64_t)H * B * C * T * F, n_w = (int64_t)H * rows.n * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(out, n_out, win, n_w) && !spans_overlap(out, n_out, wr, (int64_t)rows.n * Tw),
               "aldm_window_merge_rows: out overlaps win or wr");
    const dim3 block(256);
    if (F % 4 == 0 && (((uintptr_t)win | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(window_merge_rows_kernel<4>, dim3(win_blocks(n_out / 4)), block, 0, (hipStream_t)stream, win, wr, out, rows,
                           B, C, T, Tw, F, n_out / 4);
    } else {
        hipLaunchKernelGGL(window_merge_rows_kernel<1>, dim3(win_blocks(n_out)), block, 0, (hipStream_t)stream, win, wr, out, rows, B,
                           C, T, Tw, F, n_out);
    }
    ALDM_LAUNCH_CHECK("aldm_window_merge_rows");
    return 0;
}
