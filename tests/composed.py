"""Shared by tests/test_compose_cpu.py and tests/test_compose_gpu.py (composable guidance): the coefficient table
restated, the fp64 restatement of the compose launch with its bar, and the fp64 composition loop of a composed sampling run.

The kernel's bar.  An output element is sum_g c_g eps_g over the K+1 groups: one rounding for the first product and one per fused
multiply-add, each at most 2^-24 of the magnitude it rounds, which never exceeds sum_g |c_g eps_g|.  Measured against that sum of
magnitudes (so cancellation does not enter) the error is at most (K+1) * 2^-24 — the standard bound of a (K+1)-term fused dot
product, up to terms of order 2^-48.

The loop.  Per step K+1 SEPARATE apply_model calls (one per conditioning group, never a batched pass), the compose
e_c = sum_g c_g e_g with the table's fp32 coefficients and the guidance combine e_u + g (e_c - e_u) in fp64, then the sampler's update
in fp64 with the formulas of tests/test_guidance_gpu.py (DDIM, PLMS, DPM-Solver++ 2M) and tests/dpmpp_sde.py (the SDE solver).  On a
window plan the K+1 calls run on the window rows (torch slicing; a ring rolls; a phase rolls by the step's entry first), the compose
runs on the window rows and the merge is the fp64 overlap-add of tests/windowed.py / tests/looped.py.  Next to every fp64 step the same
step is evaluated by torch in fp32 from the same state: the worst such error is the yardstick of the sampler bars.
"""
import math

import numpy as np
import torch

import dpmpp_sde as Sd
import looped as Lp
import windowed as Wd

U = 2.0 ** -24
GS = 3.5
TINY_SHAPE = (2, 8, 16, 8)
LONG_KEY, STEPS = (40, 16, 10), 6
LONG_SHAPE = (TINY_SHAPE[0], TINY_SHAPE[1], LONG_KEY[0], TINY_SHAPE[3])

# the [(K+1), ...] group shapes of the kernel tests: 1024 elements on the 16-byte path, 1003 and 3 on the scalar one (3: fewer than a
# wave), 4100 a multiple of 4 that is no multiple of a workgroup's 1024 floats
KERNEL_SHAPES = [(3, 8, 8, 16), (3, 1, 17, 59), (2, 1, 1, 3), (1, 1, 41, 100)]
KERNEL_KS = [1, 2, 8]
# the launch caps its grid at 8192 workgroups of 256 threads: one n just above one grid pass per path, so the stride loop runs twice
GRID_THREADS = 8192 * 256
STRIDE_N = {"scalar": GRID_THREADS + 3, "vec4": 4 * GRID_THREADS + 4}


def table_by_hand(weights):
    """The [rows, K+1] fp32 table from weights [K] or [rows, K], in plain Python floats: c_0 = 1 - fsum(w), rounded to fp32 once."""
    w = [list(map(float, weights))] if not hasattr(weights[0], "__len__") else [list(map(float, r)) for r in weights]
    return torch.tensor([[float(np.float32(1.0 - math.fsum(r)))] + [float(np.float32(v)) for v in r] for r in w], dtype=torch.float32)


def kernel_weights(K, rows=1, seed=0):
    """[rows, K] seeded weights of both signs in [-1, 1.5], none 0."""
    g = torch.Generator().manual_seed(100 * K + seed)
    w = torch.rand(rows, K, generator=g, dtype=torch.float64) * 2.5 - 1.0
    return torch.where(w.abs() < 0.05, torch.full_like(w, 0.3), w)


def kernel_inputs(K, shape, seed=0):
    """eps [(K+1), *shape] fp32 host: seeded normals, group g scaled by 1 + g / 2 (the groups are not exchangeable)."""
    g = torch.Generator().manual_seed(1000 + 10 * K + seed)
    eps = torch.randn((K + 1,) + tuple(shape), generator=g)
    return (eps * (1.0 + 0.5 * torch.arange(K + 1, dtype=torch.float32)).view((-1,) + (1,) * len(shape))).contiguous()


def compose_fp64(eps, row):
    """-> (e_c = sum_g c_g eps_g in fp64, the sum of the terms' magnitudes); row: the table's K+1 fp32 coefficients."""
    e = eps.double()
    c = row.double().view((-1,) + (1,) * (eps.dim() - 1)).to(e.device)
    t = c * e
    return t.sum(0), t.abs().sum(0)


def kernel_bar(K):
    return (K + 1) * U


def off_by_one_float(t):
    """A copy of t that starts one float past a 16-byte boundary: the scalar path."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the composition loop -------------------------------------------------------------------------------------------------------------
def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


def conditioning(seed, B=TINY_SHAPE[0]):
    from oracle import cases
    _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=seed)
    return ([c.cuda() for c in ctxs], [k.cuda() for k in masks])


def group_model():
    """audio2audio.TinyModel with the group pass a LatentDiffusion has: prepare_groups / apply_model_groups over G = K+1 groups the
    way its prepare_cfg / apply_model_cfg batch two — for G = 2 the very same launches."""
    import audio2audio as A

    class GroupTinyModel(A.TinyModel):
        def prepare_groups(self, conds, uncond):
            gs = [uncond] + list(conds)
            return {"ctxs": [torch.cat([g[0][j] for g in gs]).contiguous() for j in range(len(uncond[0]))],
                    "masks": [torch.cat([g[1][j] for g in gs]).contiguous() for j in range(len(uncond[1]))], "groups": len(gs)}

        def apply_model_groups(self, x, t_row, prepared):
            G = prepared["groups"]
            eps = self.unet(x.repeat(G, 1, 1, 1).contiguous(), t_row, context_list=prepared["ctxs"],
                            context_attn_mask_list=prepared["masks"])
            return eps.view(G, x.shape[0], *eps.shape[1:])
    return GroupTinyModel()


class Passes:
    """The model side of the loop: pair(x fp32, t, i, dt) -> [e_u ; e_c] [2, b, ...] in dtype dt for loop position i.  K+1 separate
    apply_model calls on x — with `plan` on the windows of x: linear slices, a ring's rolled slices, after a roll by -phase[i] with a
    phase table — the compose in dt on those rows with row min(i, rows - 1) of `tab`, and with a plan the fp64 merge (rolled back)."""

    def __init__(self, m, conds, uncond, tab, plan=None, phase=None):
        self.m, self.groups, self.tab, self.plan, self.phase = m, [uncond] + list(conds), tab.detach().cpu(), plan, phase
        self.calls, self.last = 0, None

    def pair(self, x, t, i, dt):
        plan, phi = self.plan, 0 if self.phase is None else int(self.phase[i])
        b = x.shape[0]
        if plan is not None:
            ring = bool(getattr(plan, "ring", False))
            x = torch.roll(x, -phi, dims=2) if phi else x
            x = (Lp.ring_gather_ref if ring else Wd.gather_ref)(x.float(), plan)
        tl = torch.full((x.shape[0],), int(t), device="cuda", dtype=torch.long)
        W = x.shape[0] // b
        if self.last is not None and self.last[0] == int(t) and torch.equal(self.last[1], x):
            eps = self.last[2]   # the fp32 restatement of a step asks for the pass its fp64 form has just made
        else:
            eps = torch.stack([self.m.apply_model(x.contiguous(), tl, Wd.tile(c, W)) for c in self.groups])
            self.calls += len(self.groups)
            self.last = (int(t), x.clone(), eps)
        row = self.tab[min(i, self.tab.shape[0] - 1)]
        e = eps.to(dt)
        ec = (row.to(dt).view((-1,) + (1,) * (e.dim() - 1)).to(e.device) * e).sum(0)
        out = torch.stack([e[0], ec])
        if plan is not None:
            out = (Lp.ring_merge_fp64 if ring else Wd.merge_fp64)(out, plan)[0].to(dt)
            out = torch.roll(out, phi, dims=-2) if phi else out
        return out


def fp64_loop(kind, passes, ac, ts, xT, gs=GS, phi=0.0, eta=0.0, z=None, q=None, source=None, visits=None):
    """`kind` in ddim | plms | dpmpp | sde over the ascending timestep subset `ts` of the fp32 schedule `ac`.  The state is fp64;
    `passes.pair` sees its fp32 image.  ddim / plms run at eta = 0 (their draws are not read), sde at `eta` with the step noise z[v].
    `source` = (x0, mask): the blend of q_sample(x0, t; q[v]) in front of every step.  `visits` (DDIM): resampled inpainting — a
    renoise visit k -> k' is x = sqrt(rho) x + sqrt(1 - rho) z[v], rho = abar(k') / abar(k); the row of the weight table and the phase
    follow the step's loop position.  -> (x, the worst per-step relative error of the same step evaluated by torch in fp32)."""
    import test_guidance_gpu as G
    n = len(ts)
    time_range = np.flip(ts)
    gsf = float(torch.tensor(gs, dtype=torch.float32))
    phif = float(torch.tensor(phi, dtype=torch.float32))
    x = xT.double().cuda()
    olds, old_p0, h_last, e32 = [], None, None, 0.0
    rows = Sd.step_rows(ac, ts, eta) if kind == "sde" else None
    abar = lambda p: float(ac[ts[n - 1 - p]]) if p < n else float(ac[0])

    def guided(xx, t, i, dt):
        pair = passes.pair(xx.float(), t, i, dt)
        if phif > 0.0:
            return G.rescale_formula(pair, gsf, phif, dt)
        return pair[0] + gsf * (pair[1] - pair[0])

    for v, visit in enumerate(visits if visits is not None else [("step", i) for i in range(n)]):
        if visit[0] == "renoise":
            rho = abar(visit[2]) / abar(visit[1])
            x = math.sqrt(rho) * x + math.sqrt(1.0 - rho) * z[v].double().cuda()
            continue
        i = visit[1]
        t = time_range[i]
        index = n - i - 1
        a_t = ac[ts[index]].double()
        a_p = (ac[ts[index - 1]] if index > 0 else ac[0]).double()
        if source is not None:
            a = float(ac[int(t)])
            x0, m64 = source[0].double().cuda(), source[1].double().cuda()
            x = (math.sqrt(a) * x0 + math.sqrt(1.0 - a) * q[v].double().cuda()) * m64 + (1.0 - m64) * x
        e, e_32 = guided(x, t, i, torch.float64), guided(x, t, i, torch.float32)
        if kind == "sde":
            zi = z[v].cuda()
            x_new, p0 = Sd.sde_formula(x, e, old_p0, zi, [rows[i, j] for j in range(6)], torch.float64)
            x_32, _ = Sd.sde_formula(x.float(), e_32, old_p0, zi, [rows[i, j].float() for j in range(6)], torch.float32)
            old_p0 = p0
        elif kind == "dpmpp":
            al_t, sg_t, al_p, sg_p = a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()
            h = torch.log(al_p / sg_p) - torch.log(al_t / sg_t)
            w = torch.zeros((), dtype=torch.float64) if (i == 0 or (i == n - 1 and n < 15)) else h / (2.0 * h_last)
            c64 = [sg_t, al_t, sg_p / sg_t, -al_p * torch.expm1(-h), w]
            x_new, p0 = G.dpm_update(x, e, old_p0, c64, torch.float64)
            x_32, _ = G.dpm_update(x, e_32, old_p0, [c.float() for c in c64], torch.float32)
            old_p0, h_last = p0, h
        else:
            c64 = [(1 - a_t).sqrt(), a_t.sqrt(), (1 - a_p).sqrt(), a_p.sqrt()]
            c32 = [c.float() for c in c64]
            if kind == "plms" and i == 0:
                x_tmp, _ = G.ddim_update(x, e, c64, torch.float64)
                e_next = guided(x_tmp, time_range[min(1, n - 1)], 0, torch.float64)   # the counter has not moved: row 0
                ep, ep_32 = (e + e_next) / 2, (e_32 + e_next.float()) / 2
            elif kind == "plms":
                ep, ep_32 = G.plms_combine(e, olds[:3]), G.plms_combine(e_32, [o.float() for o in olds[:3]])
            else:
                ep, ep_32 = e, e_32
            x_new, _ = G.ddim_update(x, ep, c64, torch.float64)
            x_32, _ = G.ddim_update(x, ep_32, c32, torch.float32)
            olds.insert(0, e)
        e32 = max(e32, relmax(x_32, x_new))
        x = x_new
    return x, e32


def sampler_class(kind):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp": DPMSolverSampler, "sde": DPMSolverSDESampler}[kind]


SEED = 21


def run_sampler(kind, m, cond, uncond, S, xT, shape=TINY_SHAPE, sampler=None, gs=GS, **kw):
    """One run from the host generator seeded with SEED: eta 1 for the SDE solver (it reads its draws), 0 for the others."""
    s = sampler or sampler_class(kind)(m)
    torch.manual_seed(SEED)
    return s.sample(S, shape[0], shape[1:], cond, verbose=False, x_T=xT, eta=1.0 if kind == "sde" else 0.0,
                    unconditional_guidance_scale=gs, unconditional_conditioning=uncond, **kw)[0]


def draws(kind, shape, visits, with_q):
    """(q, z) per visit as a run seeded with SEED and given its x_T consumes them: DDIM and the SDE solver draw [q-noise,] step
    noise per visit; PLMS and DPM-Solver++ 2M are run without a source here and their draws are not read."""
    if kind in ("ddim", "sde"):
        _, q, z = Sd.host_draws(SEED, shape, visits, with_q)
        return q, z
    return None, None
