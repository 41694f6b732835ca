// windows.hip — the per-step launches of windowed (long-form) diffusion: the window gather in front of the UNet pass, the tapered,
// normalised overlap-add behind it, and the gather fused with the inpainting blend of a kept source on the long
// latent (§9f).  Each of the three is ONE kernel template over the access width V and a window geometry G: linear plans (§9e), ring
// plans whose T frames are a circle (§9g), ring plans rotated per step by a phase (§9k), and the rows of a prompt timeline (one row
// per window and prompt, the merge weighted per row and frame; §9h).  G is resolved with `if constexpr`: every instantiation
// compiles to what a hand-written kernel for its geometry compiles to (profiles/r26_window_template_isa.txt).  All are HBM-bound
// copies with at most `cover` multiply-adds (the blend: five operations) per element: 16-byte accesses along the contiguous F axis
// where F % 4 == 0 and the pointers are aligned, a scalar path otherwise, grid-stride, 64-bit indexing, fp32.  The window starts
// travel inside G as a kernel argument (aldm_window_starts / aldm_window_rows, by value): a captured step graph carries them, there
// is no device table and no copy inside a capture; every index into them is wave-uniform.  The one device table is the phase table
// of the phased ring: one int32 per visit, read with the step counter the graph already advances — a static buffer of the graph,
// refilled per job outside any capture.
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

// ---- the four geometries ------------------------------------------------------------------------------------------------------------
// A geometry is passed by value as a kernel argument and carries only what it needs: the starts, and for the phased ring its table.
// kind: which rules the starts obey (window_args_ok) and how a frame maps to a window position (window_pos); kPhased: the starts are
// rotated by a phase read per thread, once, outside the element loop (window_phase, window_start); kSkipZero: the merge skips a term
// whose weight is exactly 0.  The kernels read the fields directly and resolve the constants with `if constexpr`.
enum WinKind { WIN_LINEAR, WIN_RING, WIN_ROWS };

// window j covers the frames [s_j, s_j + Tw)
struct Linear {
    static constexpr WinKind kind = WIN_LINEAR;
    static constexpr bool kPhased = false, kSkipZero = false;
    aldm_window_starts st;
};

// seamless loops: the T frames are a circle, window j covers the frames (s_j + p) mod T.  The wrap is along T, so a
// 16-byte access along F never straddles it; it is a compare and a subtract (add), never an integer modulo: 0 <= s_j < T and
// 0 <= p < Tw <= T bound s_j + p below 2T, and t - s_j above -T.
struct Ring {
    static constexpr WinKind kind = WIN_RING;
    static constexpr bool kPhased = false, kSkipZero = false;
    aldm_window_starts st;
};

// moving window phases: a ring plan whose starts are all rotated by a phase the step counter selects.  A rigid
// rotation keeps every gap, so the plan's weights hold for every phase.  Window j covers the frames (s_j + phi + p) mod T.
struct RingPhased {
    static constexpr WinKind kind = WIN_RING;
    static constexpr bool kPhased = true, kSkipZero = false;
    aldm_window_starts st;
    const int* phase_tab;
    const int* step_idx;
    int rows;
};

// prompt timelines: a ROW is one window under one prompt, so rows may share a start.  The row starts travel by value
// (aldm_window_rows, 64 entries, 260 bytes of kernel arguments).  Rows of one window are equal copies; the gather reads each from x
// again — the long latent is R/W-th of the traffic and stays in L2.  A row whose weight at a frame is exactly 0 is skipped by the
// merge BEFORE its win element is loaded: a prompt that is silent there contributes nothing (no 0 * NaN) and costs no traffic.  The
// weight depends on (r, t) only: the skip is uniform over the F lanes of an output row.
struct Rows {
    static constexpr WinKind kind = WIN_ROWS;
    static constexpr bool kPhased = false, kSkipZero = true;
    aldm_window_rows st;
};

// The phase of this launch: 0 but for the phased ring, which chooses it ON THE DEVICE: row r = clamp(*step_idx, 0, rows - 1) of the
// int32 table (step_idx NULL: row 0), phi = clamp(phase_tab[r], 0, T - 1) — out-of-range values clamp, they do not wrap: whatever
// the table holds the launch stays in its buffers.  phi is wave-uniform.
template <class G>
__device__ __forceinline__ int window_phase(const G& g, int T) {
    if constexpr (G::kPhased) {
        int r = g.step_idx ? *g.step_idx : 0;
        r = r < 0 ? 0 : r;
        r = r < g.rows ? r : g.rows - 1;
        int phi = g.phase_tab[r];
        phi = phi < 0 ? 0 : phi;
        return phi < T ? phi : T - 1;
    } else {
        return 0;
    }
}

// the first frame of a window whose start is s: rotated by the phase where there is one (s + phi < 2T: a compare and a subtract)
template <class G>
__device__ __forceinline__ int window_start(int s, int phi, int T) {
    if constexpr (G::kPhased) {
        const int e = s + phi;
        return e >= T ? e - T : e;
    } else {
        return s;
    }
}

// the position p of frame t in a window that starts at s; false: the window does not cover t.  On a ring Tw <= T: a window covers a
// frame at most once.
template <class G>
__device__ __forceinline__ bool window_pos(int t, int s, int T, int Tw, int& p) {
    p = t - s;
    if constexpr ((G::kind == WIN_RING)) {
        if (p < 0) p += T;
        return p < Tw;
    } else {
        return !(p < 0 || p >= Tw);
    }
}

// unit i of a [..., C, T, F/V] tensor -> (fv, t, c) and the index over the leading axes
__device__ __forceinline__ int64_t unit_index(int64_t i, int FV, int T, int C, int& fv, int& t, int& c) {
    int64_t q = i / FV;
    fv = (int)(i - q * FV);
    t = (int)(q % T);
    q /= T;
    c = (int)(q % C);
    return q / C;
}

// win[(j*B + b), c, p, f] = x[b, c, (start_j + p) [mod T], f].  blockIdx.y = j; per (b, c) the Tw*F floats of a window are contiguous
// in win, and in x they are one span — on a ring at most two: frames [s, min(s + Tw, T)) and [0, s + Tw - T).  len1 = the first span
// in units; the span is picked by comparing the in-row offset with it (wave-uniform but for the one wave that holds the junction): no
// division beyond the linear form's.  per_row = Tw*F / V units per (b, c); total = B*C*per_row units per window.
template <int V, class G>
__global__ void window_gather_kernel(const float* __restrict__ x, float* __restrict__ win, G g, int T, int F, int Tw,
                                     int64_t per_row, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int j = blockIdx.y;
    const int s = window_start<G>(g.st.s[j], window_phase(g, T), T);
    const int64_t src0 = (int64_t)s * F;          // the window's offset inside a (b, c) plane of x
    const int64_t plane = (int64_t)T * F;
    float* dst = win + (int64_t)j * total * V;
    const int64_t len1 = (G::kind == WIN_RING) ? (int64_t)(Tw < T - s ? Tw : T - s) * F / V : 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bc = i / per_row, off = i - bc * per_row;
        const int64_t src = !(G::kind == WIN_RING) || off < len1 ? src0 + off * V : (off - len1) * V;
        *reinterpret_cast<vec*>(dst + i * V) = *reinterpret_cast<const vec*>(x + bc * plane + src);
    }
}

// out[h, b, c, t, f] = sum over the groups j that cover t (and, for rows, weigh it with wn != 0), ascending j, of
// wn[j, p] * win[h, j*B + b, c, p, f]: the first term a plain multiply, every later one a fused multiply-add.  Gather form: one
// thread owns an output element (V of them along F), so there are no atomics and the result does not depend on the launch geometry.
// With a phase it is the ring merge's result rolled by +phi along T, term for term.  total = H*B*C*T*(F/V) units.
template <int V, class G>
__global__ void window_merge_kernel(const float* __restrict__ win, const float* __restrict__ wn, float* __restrict__ out, G g, int B,
                                    int W, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    const int phi = window_phase(g, T);
    const int FV = F / V;
    const int R = G::kind == WIN_ROWS ? g.st.n : W;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int fv, t, c;
        const int64_t hb = unit_index(i, FV, T, C, fv, t, c);
        const int b = (int)(hb % B);
        const int64_t h = hb / B;
        vec acc = vec(0.0f);
        bool first = true;
        for (int j = 0; j < R; ++j) {
            int p;
            if (!window_pos<G>(t, window_start<G>(g.st.s[j], phi, T), T, Tw, p)) continue;
            const float wv = wn[(int64_t)j * Tw + p];
            if constexpr (G::kSkipZero) {
                if (wv == 0.0f) continue;
            }
            const vec e = *reinterpret_cast<const vec*>(win + ((((h * R + j) * B + b) * C + c) * wplane + (int64_t)p * F + fv * V));
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
// window copy of it — at most `cover` of them: win[(j*B + b), c, p, f] for the groups j that cover t at position p.  A window
// position maps to one frame, so every element of win has exactly one writer, and the windows cover [0, T) (the circle), so every
// element is written: no atomics, independent of the launch geometry.  In place on x: the owner is its element's only reader and
// writer.  The expression and its operation order are inpaint_blend_kernel's (elementwise.hip); built with -ffp-contract=off the
// launch is bitwise that kernel followed by window_gather_kernel.  The q-noise and coefficient rows are selected by the device-side
// step counter, each saturating at its table's last row (q_rows == 1: one staged draw per step).  The blend does not depend on a
// phase: x is left as the unphased form leaves it.  total = B*C*T*(F/V) units.
template <int V, class G>
__global__ void window_blend_gather_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ qnoise,
                                           const float* __restrict__ mask, const float* __restrict__ blend_coef,
                                           const int* __restrict__ step_idx, int q_rows, int coef_rows, float* __restrict__ win, G g,
                                           int B, int W, int C, int T, int Tw, int F, int64_t total) {
    typedef typename vec_of<V>::type vec;
    int s = step_idx ? *step_idx : 0;
    s = s < 0 ? 0 : s;
    const int qr = s < q_rows ? s : q_rows - 1, cr = s < coef_rows ? s : coef_rows - 1;
    const float sa = blend_coef[2 * cr], so = blend_coef[2 * cr + 1];
    const float* qn = qnoise + (int64_t)qr * total * V;
    const int phi = window_phase(g, T);
    const int FV = F / V;
    const int R = G::kind == WIN_ROWS ? g.st.n : W;
    const int64_t wplane = (int64_t)Tw * F;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int fv, t, c;
        const int64_t b = unit_index(i, FV, T, C, fv, t, c);
        const vec m = *reinterpret_cast<const vec*>(mask + i * V);
        const vec orig = sa * *reinterpret_cast<const vec*>(x0 + i * V) + so * *reinterpret_cast<const vec*>(qn + i * V);
        const vec v = orig * m + (1.0f - m) * *reinterpret_cast<const vec*>(x + i * V);
        *reinterpret_cast<vec*>(x + i * V) = v;
        for (int j = 0; j < R; ++j) {
            int p;
            if (!window_pos<G>(t, window_start<G>(g.st.s[j], phi, T), T, Tw, p)) continue;
            *reinterpret_cast<vec*>(win + (((int64_t)j * B + b) * C + c) * wplane + (int64_t)p * F + fv * V) = v;
        }
    }
}

// ---- the host side: one argument check, one launcher per operation -----------------------------------------------------------------
// The shape, and starts whose windows of Tw leave no frame without one.  Linear: strictly ascending, the last window ends at T.
// Ring: at least two windows, every start below T, the gap across the wrap in place of the last start.  Rows: non-decreasing (a
// window under several prompts repeats its start), counted by n alone.
static int window_args_ok(const char* name, WinKind kind, int n, const int* s, int B, int W, int C, int T, int Tw, int F) {
    const bool rows = kind == WIN_ROWS, ring = kind == WIN_RING;
    const char* what = rows ? "rows" : "starts";
    ALDM_CHECK(B > 0 && C > 0 && F > 0 && Tw > 0 && T >= Tw, "%s: bad shape (B=%d, C=%d, T=%d, Tw=%d, F=%d)", name, B, C, T, Tw, F);
    if (rows) {
        ALDM_CHECK(n >= 1 && n <= ALDM_MAX_ROWS, "%s: %d rows (1 <= n <= %d)", name, n, ALDM_MAX_ROWS);
    } else {
        ALDM_CHECK(W >= (ring ? 2 : 1) && W <= ALDM_MAX_WINDOWS && n == W, "%s: W=%d windows with %d starts (%d <= W == n <= %d%s)",
                   name, W, n, ring ? 2 : 1, ALDM_MAX_WINDOWS, ring ? ": a ring of one window has no window across its junction" : "");
    }
    ALDM_CHECK(s[0] == 0, "%s: %s[0]=%d must be 0", name, what, s[0]);
    for (int j = 1; j < n; ++j) {
        if (rows) {
            ALDM_CHECK(s[j] >= s[j - 1], "%s: row starts must not decrease (rows[%d]=%d after %d)", name, j, s[j], s[j - 1]);
        } else {
            ALDM_CHECK(s[j] > s[j - 1], "%s: starts must ascend (starts[%d]=%d after %d)", name, j, s[j], s[j - 1]);
        }
        if (ring) ALDM_CHECK(s[j] < T, "%s: starts[%d]=%d must lie below T=%d", name, j, s[j], T);
        ALDM_CHECK(s[j] - s[j - 1] <= Tw, "%s: gap of %d frames between %s[%d] and %s[%d] exceeds Tw=%d: frames without a %s", name,
                   s[j] - s[j - 1], what, j - 1, what, j, Tw, rows ? "row" : "window");
    }
    if (ring) {
        ALDM_CHECK(T - s[n - 1] <= Tw, "%s: gap of %d frames between starts[%d] and the wrap to frame 0 exceeds Tw=%d: frames "
                   "without a window", name, T - s[n - 1], n - 1, Tw);
    } else {
        ALDM_CHECK(s[n - 1] == T - Tw, "%s: the last %sstart %d must be T - Tw = %d", name, rows ? "row " : "", s[n - 1], T - Tw);
    }
    ALDM_CHECK((int64_t)n * B * C * Tw * F <= (1ll << 40), "%s: %lld %s elements", name, (long long)n * B * C * Tw * F,
               rows ? "row" : "window");
    return 0;
}

static inline bool spans_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

// the phase table is `rows` int32: it may share no byte with a buffer the launch writes
static inline bool phase_tab_overlaps(const RingPhased& g, const float* buf, int64_t n) {
    return spans_overlap(reinterpret_cast<const float*>(g.phase_tab), g.rows, buf, n);
}

// what a geometry checks ahead of the shape: the phased ring its table
template <class G> static int window_geom_ok(const char*, const G&) { return 0; }
static int window_geom_ok(const char* name, const RingPhased& g) {
    ALDM_CHECK(g.phase_tab, "%s: null phase table", name);
    ALDM_CHECK(g.rows >= 1, "%s: rows=%d must be >= 1", name, g.rows);
    return 0;
}

static inline bool aligned16(uintptr_t ptrs, int F) { return F % 4 == 0 && (ptrs & 15) == 0; }

template <class G>
static int window_gather_launch(const char* name, const float* x, float* win, const G& g, int B, int W, int C, int T, int Tw, int F,
                                void* stream) {
    ALDM_CHECK(x && win, "%s: null pointer", name);
    if (window_geom_ok(name, g) != 0 || window_args_ok(name, G::kind, g.st.n, g.st.s, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(x, n_x, win, n_w), "%s: win overlaps x", name);
    if constexpr (G::kPhased) ALDM_CHECK(!phase_tab_overlaps(g, win, n_w), "%s: win overlaps phase_tab", name);
    const int64_t per_window = (int64_t)B * C * Tw * F;
    if (aligned16((uintptr_t)x | (uintptr_t)win, F)) {
        hipLaunchKernelGGL((window_gather_kernel<4, G>), dim3(win_blocks(per_window / 4), W), dim3(256), 0, (hipStream_t)stream, x,
                           win, g, T, F, Tw, (int64_t)Tw * F / 4, per_window / 4);
    } else {
        hipLaunchKernelGGL((window_gather_kernel<1, G>), dim3(win_blocks(per_window), W), dim3(256), 0, (hipStream_t)stream, x, win,
                           g, T, F, Tw, (int64_t)Tw * F, per_window);
    }
    ALDM_LAUNCH_CHECK(name);
    return 0;
}

template <class G>
static int window_blend_gather_launch(const char* name, float* x, const float* x0, const float* qnoise, const float* mask,
                                      const float* blend_coef, const int* step_idx, int q_rows, int coef_rows, float* win, const G& g,
                                      int B, int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(x && x0 && qnoise && mask && blend_coef && win, "%s: null pointer", name);
    if (window_geom_ok(name, g) != 0 || window_args_ok(name, G::kind, g.st.n, g.st.s, B, W, C, T, Tw, F) != 0) return -1;
    ALDM_CHECK(q_rows >= 1 && coef_rows >= 1, "%s: q_rows=%d and coef_rows=%d must be >= 1", name, q_rows, coef_rows);
    const int64_t n_x = (int64_t)B * C * T * F, n_w = (int64_t)W * B * C * Tw * F, n_q = (int64_t)q_rows * n_x;
    ALDM_CHECK(!spans_overlap(win, n_w, x, n_x) && !spans_overlap(win, n_w, x0, n_x) && !spans_overlap(win, n_w, qnoise, n_q) &&
               !spans_overlap(win, n_w, mask, n_x), "%s: win overlaps x, x0, qnoise or mask", name);
    ALDM_CHECK(!spans_overlap(x, n_x, x0, n_x) && !spans_overlap(x, n_x, qnoise, n_q) && !spans_overlap(x, n_x, mask, n_x),
               "%s: x overlaps x0, qnoise or mask", name);
    if constexpr (G::kPhased)
        ALDM_CHECK(!phase_tab_overlaps(g, win, n_w) && !phase_tab_overlaps(g, x, n_x), "%s: win or x overlaps phase_tab", name);
    if (aligned16((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)qnoise | (uintptr_t)mask | (uintptr_t)win, F)) {
        hipLaunchKernelGGL((window_blend_gather_kernel<4, G>), dim3(win_blocks(n_x / 4)), dim3(256), 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, g, B, W, C, T, Tw, F, n_x / 4);
    } else {
        hipLaunchKernelGGL((window_blend_gather_kernel<1, G>), dim3(win_blocks(n_x)), dim3(256), 0, (hipStream_t)stream, x, x0,
                           qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win, g, B, W, C, T, Tw, F, n_x);
    }
    ALDM_LAUNCH_CHECK(name);
    return 0;
}

// wname: what the entry's messages call the weights
template <class G>
static int window_merge_launch(const char* name, const char* wname, const float* win, const float* wn, float* out, const G& g, int H,
                               int B, int W, int C, int T, int Tw, int F, void* stream) {
    ALDM_CHECK(win && wn && out, "%s: null pointer", name);
    if (window_geom_ok(name, g) != 0) return -1;
    ALDM_CHECK(H == 1 || H == 2, "%s: H=%d: 1, or 2 for the [uncond ; cond] pair", name, H);
    if (window_args_ok(name, G::kind, g.st.n, g.st.s, B, W, C, T, Tw, F) != 0) return -1;
    const int64_t n_out = (int64_t)H * B * C * T * F, n_w = (int64_t)H * W * B * C * Tw * F;
    ALDM_CHECK(!spans_overlap(out, n_out, win, n_w) && !spans_overlap(out, n_out, wn, (int64_t)W * Tw), "%s: out overlaps win or %s",
               name, wname);
    if constexpr (G::kPhased) ALDM_CHECK(!phase_tab_overlaps(g, out, n_out), "%s: out overlaps phase_tab", name);
    if (aligned16((uintptr_t)win | (uintptr_t)out, F)) {
        hipLaunchKernelGGL((window_merge_kernel<4, G>), dim3(win_blocks(n_out / 4)), dim3(256), 0, (hipStream_t)stream, win, wn, out,
                           g, B, W, C, T, Tw, F, n_out / 4);
    } else {
        hipLaunchKernelGGL((window_merge_kernel<1, G>), dim3(win_blocks(n_out)), dim3(256), 0, (hipStream_t)stream, win, wn, out, g,
                           B, W, C, T, Tw, F, n_out);
    }
    ALDM_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace aldm

using namespace aldm;

// ---- the entries: each names itself and its geometry; a row entry's W is its row count --------------------------------------------
extern "C" int aldm_window_gather(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F,
                                  void* stream) {
    return window_gather_launch("aldm_window_gather", x, win, Linear{starts}, B, W, C, T, Tw, F, stream);
}

extern "C" int aldm_window_blend_gather(float* x, const float* x0, const float* qnoise, const float* mask, const float* blend_coef,
                                        const int* step_idx, int q_rows, int coef_rows, float* win, aldm_window_starts starts, int B,
                                        int W, int C, int T, int Tw, int F, void* stream) {
    return window_blend_gather_launch("aldm_window_blend_gather", x, x0, qnoise, mask, blend_coef, step_idx, q_rows, coef_rows, win,
                                      Linear{starts}, B, W, C, T, Tw, F, stream);
}

extern "C" int aldm_window_merge(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W, int C,
                                 int T, int Tw, int F, void* stream) {
    return window_merge_launch("aldm_window_merge", "wn", win, wn, out, Linear{starts}, H, B, W, C, T, Tw, F, stream);
}

// the ring entries (ABI v20): the argument lists of the linear ones
extern "C" int aldm_window_gather_ring(const float* x, float* win, aldm_window_starts starts, int B, int W, int C, int T, int Tw,
                                       int F, void* stream) {
    return window_gather_launch("aldm_window_gather_ring", x, win, Ring{starts}, B, W, C, T, Tw, F, stream);
}

extern "C" int aldm_window_blend_gather_ring(float* x, const float* x0, const float* qnoise, const float* mask,
                                             const float* blend_coef, const int* step_idx, int q_rows, int coef_rows, float* win,
                                             aldm_window_starts starts, int B, int W, int C, int T, int Tw, int F, void* stream) {
    return window_blend_gather_launch("aldm_window_blend_gather_ring", x, x0, qnoise, mask, blend_coef, step_idx, q_rows, coef_rows,
                                      win, Ring{starts}, B, W, C, T, Tw, F, stream);
}

extern "C" int aldm_window_merge_ring(const float* win, const float* wn, float* out, aldm_window_starts starts, int H, int B, int W,
                                      int C, int T, int Tw, int F, void* stream) {
    return window_merge_launch("aldm_window_merge_ring", "wn", win, wn, out, Ring{starts}, H, B, W, C, T, Tw, F, stream);
}

// the phased ring entries (ABI v25, moving window phases): the ring entries' checks, plus the phase table
extern "C" int aldm_window_gather_ring_phased(const float* x, float* win, aldm_window_starts starts, const int* phase_tab,
                                              const int* step_idx, int rows, int B, int W, int C, int T, int Tw, int F, void* stream) {
    return window_gather_launch("aldm_window_gather_ring_phased", x, win, RingPhased{starts, phase_tab, step_idx, rows}, B, W, C, T,
                                Tw, F, stream);
}

extern "C" int aldm_window_blend_gather_ring_phased(float* x, const float* x0, const float* qnoise, const float* mask,
                                                    const float* blend_coef, const int* step_idx, int q_rows, int coef_rows,
                                                    float* win, aldm_window_starts starts, const int* phase_tab, int rows, int B,
                                                    int W, int C, int T, int Tw, int F, void* stream) {
    return window_blend_gather_launch("aldm_window_blend_gather_ring_phased", x, x0, qnoise, mask, blend_coef, step_idx, q_rows,
                                      coef_rows, win, RingPhased{starts, phase_tab, step_idx, rows}, B, W, C, T, Tw, F, stream);
}

extern "C" int aldm_window_merge_ring_phased(const float* win, const float* wn, float* out, aldm_window_starts starts,
                                             const int* phase_tab, const int* step_idx, int rows, int H, int B, int W, int C, int T,
                                             int Tw, int F, void* stream) {
    return window_merge_launch("aldm_window_merge_ring_phased", "wn", win, wn, out, RingPhased{starts, phase_tab, step_idx, rows}, H,
                               B, W, C, T, Tw, F, stream);
}

// the row entries (ABI v22, prompt timelines): rows = (window, prompt) pairs, starts non-decreasing
extern "C" int aldm_window_gather_rows(const float* x, float* win, aldm_window_rows rows, int B, int C, int T, int Tw, int F,
                                       void* stream) {
    return window_gather_launch("aldm_window_gather_rows", x, win, Rows{rows}, B, rows.n, C, T, Tw, F, stream);
}

extern "C" int aldm_window_blend_gather_rows(float* x, const float* x0, const float* qnoise, const float* mask,
                                             const float* blend_coef, const int* step_idx, int q_rows, int coef_rows, float* win,
                                             aldm_window_rows rows, int B, int C, int T, int Tw, int F, void* stream) {
    return window_blend_gather_launch("aldm_window_blend_gather_rows", x, x0, qnoise, mask, blend_coef, step_idx, q_rows, coef_rows,
                                      win, Rows{rows}, B, rows.n, C, T, Tw, F, stream);
}

extern "C" int aldm_window_merge_rows(const float* win, const float* wr, float* out, aldm_window_rows rows, int H, int B, int C, int T,
                                      int Tw, int F, void* stream) {
    return window_merge_launch("aldm_window_merge_rows", "wr", win, wr, out, Rows{rows}, H, B, rows.n, C, T, Tw, F,
                               stream);
}
