"""The launch sequence and the host draws of the three samplers (DDIM, PLMS, DPM-Solver++(2M)), pinned: a guard for changes that
move code between ddim.py, plms.py, dpm_solver.py and sampling.py without meaning to change what a run does.

Every run is on the tiny UNet at TINY_SHAPE with S = 4 (four steps: timesteps 751, 501, 251, 1), under ALDM_NO_GRAPH=1 and
ALDM_NOISE_THREAD=0, so every step executes its Python closure on the calling thread.  Two lists are recorded:
  * launches: (name, value of the device step counter where the op takes one, else None), of the `ops` functions a sampling loop
    calls and of the model's apply_model / apply_model_cfg;
  * host draws: the shape of every `torch.randn` call.
The expected lists below were written down from the three loops as they stood before sampling.py existed, not recorded: one
string per run, steps separated by `|`, `name@k` = the launch found the step counter at k.  After each run the host generator must
be where replaying the recorded draws from the same seed leaves it.
"""
import pytest
import torch

from oracle import cases, weights

pytestmark = pytest.mark.gpu
GS, PHI, S, SEED = 3.5, 0.7, 4, 1234
TINY_SHAPE = (2, 8, 16, 8)
RANDN = torch.randn   # the real one: the recorder below replaces the module attribute

NAMES = {"U": "apply_model", "U2": "apply_model_cfg", "resc": "cfg_rescale_indexed", "ddim": "ddim_step_indexed",
         "first": "plms_first_step", "plms": "plms_step_indexed", "dpm": "dpmpp_step_indexed", "adv": "step_advance",
         "blend": "inpaint_blend"}
COUNTER_ARG = {"ddim_step_indexed": 4, "plms_step_indexed": 4, "dpmpp_step_indexed": 4, "cfg_rescale_indexed": 3, "step_advance": 0}

LAUNCHES = {
    # DDIM: UNet pass -> [rescale] -> step -> advance, the blend in front
    ("ddim", "cfg"): "U2 ddim@0 adv@0 | U2 ddim@1 adv@1 | U2 ddim@2 adv@2 | U2 ddim@3 adv@3",
    ("ddim", "rescale"): "U2 resc@0 ddim@0 adv@0 | U2 resc@1 ddim@1 adv@1 | U2 resc@2 ddim@2 adv@2 | U2 resc@3 ddim@3 adv@3",
    ("ddim", "plain"): "U ddim@0 adv@0 | U ddim@1 adv@1 | U ddim@2 adv@2 | U ddim@3 adv@3",
    ("ddim", "masked"): "blend U2 ddim@0 adv@0 | blend U2 ddim@1 adv@1 | blend U2 ddim@2 adv@2 | blend U2 ddim@3 adv@3",
    ("ddim", "t_start"): "U2 ddim@0 adv@0 | U2 ddim@1 adv@1",
    # PLMS: step 0 is two passes and two first-step launches (its rescale launches take no counter: row 0), then one pass per step
    ("plms", "cfg"): "U2 first U2 first adv@0 | U2 plms@1 adv@1 | U2 plms@2 adv@2 | U2 plms@3 adv@3",
    ("plms", "rescale"): "U2 resc first U2 resc first adv@0 | U2 resc@1 plms@1 adv@1 | U2 resc@2 plms@2 adv@2 | U2 resc@3 plms@3 adv@3",
    ("plms", "plain"): "U first U first adv@0 | U plms@1 adv@1 | U plms@2 adv@2 | U plms@3 adv@3",
    ("plms", "masked"): "blend U2 first U2 first adv@0 | blend U2 plms@1 adv@1 | blend U2 plms@2 adv@2 | blend U2 plms@3 adv@3",
    ("plms", "t_start"): "U2 first U2 first adv@0 | U2 plms@1 adv@1",
    # DPM-Solver++(2M): every step, step 0 included, is the same sequence
    ("dpmpp", "cfg"): "U2 dpm@0 adv@0 | U2 dpm@1 adv@1 | U2 dpm@2 adv@2 | U2 dpm@3 adv@3",
    ("dpmpp", "rescale"): "U2 resc@0 dpm@0 adv@0 | U2 resc@1 dpm@1 adv@1 | U2 resc@2 dpm@2 adv@2 | U2 resc@3 dpm@3 adv@3",
    ("dpmpp", "plain"): "U dpm@0 adv@0 | U dpm@1 adv@1 | U dpm@2 adv@2 | U dpm@3 adv@3",
    ("dpmpp", "masked"): "blend U2 dpm@0 adv@0 | blend U2 dpm@1 adv@1 | blend U2 dpm@2 adv@2 | blend U2 dpm@3 adv@3",
    ("dpmpp", "t_start"): "U2 dpm@0 adv@0 | U2 dpm@1 adv@1",
}

# Host draws, every one of TINY_SHAPE.  DDIM: x_T, then per step [the q_sample noise of the blend,] the step noise.  PLMS: x_T, per
# step [the q_sample noise,] one discarded noise_like, two in step 0.  DPM-Solver++: x_T and the q_sample noise, nothing else.
# `t_start`: x_T is given, so it is not drawn.
DRAWS = {
    ("ddim", "cfg"): 1 + 4, ("ddim", "rescale"): 1 + 4, ("ddim", "plain"): 1 + 4, ("ddim", "masked"): 1 + 4 * 2, ("ddim", "t_start"): 2,
    ("plms", "cfg"): 1 + 2 + 3, ("plms", "rescale"): 1 + 2 + 3, ("plms", "plain"): 1 + 2 + 3, ("plms", "masked"): 1 + 3 + 3 * 2,
    ("plms", "t_start"): 2 + 1,
    ("dpmpp", "cfg"): 1, ("dpmpp", "rescale"): 1, ("dpmpp", "plain"): 1, ("dpmpp", "masked"): 1 + 4, ("dpmpp", "t_start"): 0,
}


class TinyModel:
    """test_plms_gpu.TinyModel: what a sampler touches on its model, over the tiny UNet; conditioning = (contexts, masks)."""
    num_timesteps = 1000

    def __init__(self):
        from audioldm2_amd.unet import UNetModel
        self.unet = UNetModel(**cases.UNET_TINY)
        self.unet.load_state_dict(weights.make_state_dict(weights.shapes_of(self.unet), seed=0))
        self.unet.cuda()
        betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()

    def apply_model(self, x, t, cond):
        return self.unet(x.contiguous(), t, context_list=cond[0], context_attn_mask_list=cond[1])

    def prepare_cfg(self, cond, uncond):
        return {"ctxs": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[0], cond[0])],
                "masks": [torch.cat([u, c]).contiguous() for u, c in zip(uncond[1], cond[1])]}

    def apply_model_cfg(self, x, t2, cond=None, uncond=None, prepared=None):
        p = prepared or self.prepare_cfg(cond, uncond)
        eps = self.unet(x.repeat(2, 1, 1, 1).contiguous(), t2, context_list=p["ctxs"], context_attn_mask_list=p["masks"])
        return eps.view(2, x.shape[0], *eps.shape[1:])


def parse(text):
    out = []
    for tok in text.replace("|", " ").split():
        name, _, k = tok.partition("@")
        out.append((NAMES[name], int(k) if k else None))
    return out


@pytest.fixture(scope="module")
def tiny():
    m = TinyModel()
    B = TINY_SHAPE[0]
    _, _, ctxs, masks, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=1)
    _, _, uctx, umask, _ = cases.unet_inputs(cases.UNET_TINY, B, 16, 8, 12, seed=2)
    cond = ([c.cuda() for c in ctxs], [k.cuda() for k in masks])
    uncond = ([c.cuda() for c in uctx], [k.cuda() for k in umask])
    return m, cond, uncond


def make_sampler(kind, m):
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.dpm_solver import DPMSolverSampler
    from audioldm2_amd.plms import PLMSSampler
    return {"ddim": DDIMSampler, "plms": PLMSSampler, "dpmpp": DPMSolverSampler}[kind](m)


@pytest.fixture
def record(tiny, monkeypatch):
    """-> start(): from that call on, launches and draws are appended to the two lists it returns."""
    from audioldm2_amd import ops
    monkeypatch.setenv("ALDM_NO_GRAPH", "1")
    monkeypatch.setenv("ALDM_NOISE_THREAD", "0")
    m = tiny[0]

    def start():
        launches, draws = [], []

        def wrap(owner, name):
            fn = getattr(owner, name)
            pos = COUNTER_ARG.get(name)

            def wrapped(*a, **k):
                idx = None if pos is None else (a[pos] if len(a) > pos else k.get("step_idx"))
                launches.append((name, None if idx is None else int(idx.item())))
                return fn(*a, **k)
            monkeypatch.setattr(owner, name, wrapped)
        for name in NAMES.values():
            wrap(m if name.startswith("apply_model") else ops, name)

        def randn_rec(*a, **k):
            draws.append(tuple(a[0]) if not isinstance(a[0], int) else tuple(a))
            return RANDN(*a, **k)
        monkeypatch.setattr(torch, "randn", randn_rec)
        return launches, draws
    return start


def generator_state_after(draws):
    torch.manual_seed(SEED)
    for shape in list(draws):
        RANDN(shape)
    return torch.get_rng_state()


@pytest.mark.parametrize("case", ["cfg", "rescale", "plain", "masked", "t_start"])
@pytest.mark.parametrize("kind", ["ddim", "plms", "dpmpp"])
def test_launches_and_draws_of_a_run(tiny, record, kind, case):
    m, cond, uncond = tiny
    kw = dict(unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    if case == "rescale":
        kw["guidance_rescale"] = PHI
    elif case == "plain":
        kw = {}
    elif case == "masked":
        g = torch.Generator().manual_seed(7)
        mask = torch.ones(TINY_SHAPE[0], 1, *TINY_SHAPE[2:])
        mask[:, :, 4:12, :] = 0
        kw.update(mask=mask, x0=torch.randn(TINY_SHAPE, generator=g))
    elif case == "t_start":
        x_T = torch.randn(TINY_SHAPE, generator=torch.Generator().manual_seed(3)).cuda()
        given = x_T.clone()
        kw.update(x_T=x_T, t_start=2)
    s = make_sampler(kind, m)
    assert not s.use_graph
    launches, draws = record()
    torch.manual_seed(SEED)
    out, inter = s.sample(S, TINY_SHAPE[0], TINY_SHAPE[1:], cond, verbose=False, eta=0.0, **kw)
    state = torch.get_rng_state()
    print(f"{kind} {case}: {len(launches)} launches, {len(draws)} draws")
    assert launches == parse(LAUNCHES[kind, case])
    assert draws == [TINY_SHAPE] * DRAWS[kind, case]
    assert torch.equal(state, generator_state_after(draws))
    assert out.is_cuda and tuple(out.shape) == TINY_SHAPE and bool(torch.isfinite(out).all())
    if case == "t_start":
        first = inter["x_inter"][0]
        # the given device tensor itself: never copied through the host
        assert first.is_cuda and first.data_ptr() == x_T.data_ptr() and torch.equal(first, given)
        assert len(inter["x_inter"]) == 1 + 2    # index 1 is the run's first step, index 0 is logged always


@pytest.mark.parametrize("give_x_T", [True, False], ids=["x_T given", "x_T drawn"])
@pytest.mark.parametrize("kind", ["ddim", "plms", "dpmpp"])
def test_zero_steps_launch_nothing_and_return_x_T(tiny, record, kind, give_x_T):
    """`timesteps=1` on a 4-entry schedule keeps int(min(1 / 4, 1) * 4) - 1 = 0 entries: no launch, x_T comes back bitwise, and the
    generator is consumed by the x_T draw alone, when there is one."""
    m, cond, uncond = tiny
    s = make_sampler(kind, m)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    x_T = torch.randn(TINY_SHAPE, generator=torch.Generator().manual_seed(3)) if give_x_T else None
    loop = getattr(s, {"ddim": "ddim_sampling", "plms": "plms_sampling", "dpmpp": "dpm_sampling"}[kind])
    launches, draws = record()
    torch.manual_seed(SEED)
    out, inter = loop(cond, TINY_SHAPE, x_T=x_T, timesteps=1, unconditional_guidance_scale=GS, unconditional_conditioning=uncond)
    state = torch.get_rng_state()
    assert launches == []
    assert draws == ([] if give_x_T else [TINY_SHAPE])
    assert torch.equal(state, generator_state_after(draws))
    if not give_x_T:
        torch.manual_seed(SEED)
        x_T = RANDN(TINY_SHAPE)
    assert out.is_cuda and torch.equal(out.cpu(), x_T)
    assert len(inter["x_inter"]) == 1 and torch.equal(inter["x_inter"][0], out) and torch.equal(inter["pred_x0"][0], out)
