"""Composable guidance without a GPU: the entry point and its host checks, the coefficient table, the sampler-side
refusals, and every refusal of the pipeline with the host generator untouched."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import composed as Cp


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    from audioldm2_amd import lib, ops, sampling
    assert lib.ABI_VERSION >= 27      # the entry point arrived with ABI 27
    l = lib.load()
    assert l.aldm_version() == lib.ABI_VERSION
    assert "aldm_cfg_compose_indexed" in lib.EXPORTED_SYMBOLS and hasattr(l, "aldm_cfg_compose_indexed")
    assert ops.MAX_COMPOSE == sampling.MAX_COMPOSE == 8
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aldm_hip.h")) as f:
        header = f.read()
    assert "#define ALDM_MAX_COMPOSE 8" in header and "int aldm_cfg_compose_indexed(" in header


def test_entry_validates_before_launch():
    """aldm_cfg_compose_indexed refuses null pointers, K outside [1, 8], rows < 1, pair outside {0, 1}, n outside (0, 2^40], an out
    that overlaps eps other than out == eps, and an out that overlaps the weight table — before any launch: observable without a GPU
    (the pointers are never dereferenced)."""
    from audioldm2_amd import lib
    l = lib.load()
    p = lambda a: ctypes.c_void_p(a)
    eps, out, tab, idx = 1 << 24, 1 << 28, 1 << 30, 1 << 31
    n, K, rows = 64, 2, 3
    fn = l.aldm_cfg_compose_indexed
    for k in (0, 1, 2):
        args = [p(eps), p(out), p(tab), p(idx), rows, K, 1, n]
        args[k] = None
        assert fn(*args, None) != 0, k
        assert "null pointer" in l.aldm_last_error().decode(), k

    def refused(msg, **kw):
        a = dict(eps=p(eps), out=p(out), tab=p(tab), idx=p(idx), rows=rows, K=K, pair=1, n=n)
        a.update(kw)
        assert fn(a["eps"], a["out"], a["tab"], a["idx"], a["rows"], a["K"], a["pair"], a["n"], None) != 0, kw
        assert msg in l.aldm_last_error().decode(), (kw, l.aldm_last_error())
    refused("K=0", K=0)
    refused("K=9", K=9)
    refused("K=-1", K=-1)
    refused("rows=0", rows=0)
    refused("rows=-2", rows=-2)
    refused("pair=2", pair=2)
    refused("pair=-1", pair=-1)
    refused("n=0", n=0)
    refused("n=-4", n=-4)
    refused(f"n={(1 << 40) + 1}", n=(1 << 40) + 1)
    # out against eps [(K+1), n]: anything but out == eps that shares a byte — inside a group, one group on, straddling either end
    for at in (eps + 4, eps + 4 * n, eps + 4 * (K + 1) * n - 4, eps - 4 * (2 * n - 1), eps - 4):
        refused("out overlaps eps", out=p(at))
    # pair = 0 writes n floats only: an out that ends where eps begins is fine for it and refused for the pair ... without a GPU the
    # accepted side cannot be launched, so only the refused side is called
    refused("out overlaps eps", out=p(eps - 4 * n - 4), pair=1)
    # out against the weight table [rows, K+1]
    for at in (tab, tab + 4 * (rows * (K + 1) - 1), tab - 4 * (2 * n - 1)):
        refused("out overlaps w_tab", out=p(at))
    refused("out overlaps w_tab", eps=p(tab - 4 * n), out=p(tab - 4 * n))        # in place, its pair's second half runs into the table
    with pytest.raises(RuntimeError, match="out overlaps w_tab"):
        lib.check(1, "cfg_compose_indexed")


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_table_c0_comes_from_the_fp64_sum():
    from audioldm2_amd.sampling import Composed, compose_table
    # fp32 arithmetic would give 1 - (0.1f + 0.2f + 0.3f) != float32(1 - 0.6): the rounding happens once, after the fp64 sum
    w = [0.1, 0.2, 0.3]
    tab = compose_table(Composed([None] * 3, w).weights)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (1, 4)
    assert torch.equal(tab, Cp.table_by_hand(w))
    assert float(tab[0, 0]) == float(np.float32(1.0 - math.fsum(w)))
    f32 = np.float32(1.0) - (np.float32(0.1) + np.float32(0.2) + np.float32(0.3))
    assert float(tab[0, 0]) != float(f32)
    # K = 1, w = 1: {0, 1} exactly — the sampler then makes the plain job
    assert compose_table(Composed([None], [1.0]).weights).tolist() == [[0.0, 1.0]]
    # weights that sum to 1: c_0 is exactly 0, the unconditional group is not read
    assert float(compose_table(Composed([None] * 2, [1.5, -0.5]).weights)[0, 0]) == 0.0
    for K in Cp.KERNEL_KS:
        w = Cp.kernel_weights(K, rows=3).tolist()
        assert torch.equal(compose_table(Composed([None] * K, w).weights, 3), Cp.table_by_hand(w))


def test_table_rows_scalar_schedule_cut_and_visits():
    from audioldm2_amd.sampling import Composed, compose_table, resample_visits
    S, K = 6, 2
    sched = [[1.0 - 0.1 * i, -0.5 + 0.2 * i] for i in range(S)]
    by_hand = Cp.table_by_hand(sched)
    c = Composed([None] * K, sched)
    assert tuple(compose_table(Composed([None] * K, [1.0, -0.5]).weights, S).shape) == (1, 3)          # a scalar weight: one row
    assert torch.equal(compose_table(c.weights, S), by_hand)                                            # a schedule: total_steps rows
    # a run of the schedule's last 4 steps (audio-to-audio, t_start) reads the last 4 rows
    assert torch.equal(compose_table(c.weights, 4, None, S), by_hand[2:])
    visits = resample_visits(S, 2, 2)
    rows = [v[1] if v[0] == "step" else v[2] for v in visits]
    assert len(visits) > S
    tab = compose_table(c.weights, S, visits)
    assert tuple(tab.shape) == (len(visits), K + 1) and torch.equal(tab, by_hand[rows])                # resample=: one row per visit
    # a renoise visit takes the next step visit's row (blend_coef's rule)
    for v, nxt in zip(range(len(visits)), range(1, len(visits))):
        if visits[v][0] == "renoise":
            assert visits[nxt][0] == "step" and torch.equal(tab[v], tab[nxt])
    # a constant weight stays one row under visits
    assert tuple(compose_table(Composed([None] * K, [1.0, -0.5]).weights, S, visits).shape) == (1, 3)
    for bad_steps, sl in ((5, None), (5, 7), (7, 6)):
        with pytest.raises(ValueError, match="weight schedule has 6 rows"):
            compose_table(c.weights, bad_steps, None, sl)


def test_composed_refuses_what_it_cannot_run():
    from audioldm2_amd.sampling import Composed
    for conds, w, msg in (([], [], "between 1 and 8"), ([None] * 9, [1.0] * 9, "between 1 and 8"),
                          ([None] * 2, [1.0], r"shape \[2\]"), ([None] * 2, [[1.0, 2.0, 3.0]], r"shape \[2\]"),
                          ([None] * 2, [1.0, float("nan")], "finite"), ([None] * 2, [float("inf"), 1.0], "finite"),
                          ([None] * 2, [0.0, 0.0], "every weight is 0"), ([None] * 2, [[1.0, 0.5], [0.0, 0.0]], "every weight is 0"),
                          ([None] * 2, ["a", "b"], "numbers"), ([None] * 2, np.zeros((0, 2)), r"shape \[2\]")):
        with pytest.raises(ValueError, match=msg):
            Composed(conds, w)
    assert len(Composed([None] * 8, [1.0] * 8)) == 8
    assert Composed([None] * 2, [0.0, -1.0]).weights.tolist() == [0.0, -1.0]     # one zero weight is legal: the kernel skips it


class _Schedule:
    """What plan_run reads of a model before it touches the GPU."""
    num_timesteps = 1000

    def __init__(self):
        betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()


def test_plan_run_refuses_a_composed_run_before_the_first_draw():
    from audioldm2_amd.ddim import DDIMSampler
    from audioldm2_amd.sampling import Composed
    from audioldm2_amd.windows import prompt_weights, row_plan, window_plan
    s = DDIMSampler(_Schedule())
    s.make_schedule(6, ddim_eta=0.0, verbose=False)
    assert len(s.ddim_timesteps) == 7
    table = lambda n, cfg: torch.zeros(n, 8)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    c = Composed([None] * 2, [1.0, -0.5])
    with pytest.raises(ValueError, match="unconditional conditioning"):
        s.plan_run(c, (2, 8, 16, 8), None, None, None, table, 3.5, None, 0.0, None, None)
    with pytest.raises(ValueError, match="weight schedule has 5 rows"):
        s.plan_run(Composed([None] * 2, [[1.0, 0.5]] * 5), (2, 8, 16, 8), None, None, None, table, 3.5, object(), 0.0, None, None)
    rp = row_plan(window_plan(40, 16, 10), prompt_weights(40, [20], 4))
    with pytest.raises(ValueError, match="row plan"):
        s.plan_run(c, (2, 8, 40, 8), None, None, None, table, 3.5, object(), 0.0, None, None, windows=rp)
    assert torch.equal(torch.get_rng_state(), state)


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
class _NoGpu:
    """Stands where a LatentDiffusion would: what the entry points read before they touch the GPU; anything else raises."""
    latent_t_size, latent_t_per_second, first_stage_key, num_timesteps = 256, 25.6, "fbank", 1000

    class first_stage_model:
        class encoder:
            num_resolutions = 3

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the arguments were checked")


def _ld_stub():
    from audioldm2_amd.pipeline import LatentDiffusion

    class Stub(_NoGpu):
        pass
    for name in ("long_form_plans", "generate_batch", "generate_batch_masked", "generate_batch_from_audio", "generate_batch_long",
                 "generate_batch_long_from_audio", "check_latent_t"):
        fn = inspect.getattr_static(LatentDiffusion, name)
        fn = fn.__func__ if isinstance(fn, staticmethod) else fn
        fn = getattr(fn, "__wrapped__", fn)
        setattr(Stub, name, staticmethod(fn) if name == "check_latent_t" else fn)
    return Stub()


MIX = [("rain on a tin roof", 1.0), ("distant thunder", 0.6), ("traffic", -0.4)]
# what every entry point refuses of a compose= list: (keywords over the good call, the message)
BAD_LISTS = [(dict(compose=[]), "non-empty list"), (dict(compose=[("p", 1.0)] * 9), "at most 8"),
             (dict(compose=[("a", float("nan")), ("b", 1.0)]), "finite"), (dict(compose=[("a", float("inf"))]), "finite"),
             (dict(compose=[("a", 1.0), ("b", "x")]), "finite number or a list"), (dict(compose=[("a",)]), "entry is"),
             (dict(compose=[(1.0, "a")]), "entry is"), (dict(compose=[("a", 1.0, 3)]), "entry is"),
             (dict(compose=[("a", 0.0), ("b", 0.0)]), "every weight is 0"),
             (dict(compose=[("a", [1.0, 0.0, 1.0, 1.0]), ("b", [0.5, 0.0, 0.5, 0.5])]), "every weight is 0"),
             (dict(compose=[("a", [1.0, 1.0, 1.0]), ("b", 0.5)]), "3 entries for ddim_steps=4"),
             (dict(compose=MIX, ddim_steps=None), "ddim_steps"), (dict(compose=MIX, guidance_scale=1.0), "unconditional conditioning"),
             (dict(compose=MIX, text="rain"), "pass text=None"), (dict(compose=MIX, transcription="hello"), "pass text=None")]


def test_entry_points_refuse_a_bad_compose_before_any_draw_or_gpu_work():
    from audioldm2_amd.pipeline import extend_audio, text_to_audio, text_to_audio_long
    ld = _ld_stub()
    wav = np.zeros(16000, dtype=np.float32)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    short = dict(n_candidate_gen_per_text=1)
    calls = {"text_to_audio": (lambda text, **kw: text_to_audio(ld, text, **kw), short),
             "text_to_audio_long": (lambda text, **kw: text_to_audio_long(ld, text, 30, **kw), {}),
             "extend_audio": (lambda text, **kw: extend_audio(ld, text, wav, 30, **kw), {})}
    for name, (call, base) in calls.items():
        for kw, msg in BAD_LISTS:
            args = dict(dict(base, text=None, ddim_steps=4), **kw)
            with pytest.raises(ValueError, match=msg):
                call(args.pop("text"), **args)
        if base:   # the entry points with candidates: the default of three per text is refused, like any count above one
            for n in (None, 2):
                with pytest.raises(ValueError, match="n_candidate_gen_per_text"):
                    call(None, compose=MIX, ddim_steps=4, **({} if n is None else {"n_candidate_gen_per_text": n}))
        else:      # the long-form entry points: not together with a timeline
            with pytest.raises(ValueError, match="timeline"):
                call(None, compose=MIX, ddim_steps=4, timeline=[(0.0, "rain"), (12.0, "thunder")])
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn, the seed was not set
    assert ld.latent_t_size == 256


def test_generate_batch_methods_refuse_a_bad_composed_job_before_any_draw():
    from audioldm2_amd.pipeline import make_batch_for_text_to_audio
    ld = _ld_stub()
    batches = [make_batch_for_text_to_audio(p) for p, _ in MIX]
    w = [1.0, 0.6, -0.4]
    torch.manual_seed(5)
    state = torch.get_rng_state()
    jobs = {"generate_batch": lambda b, **kw: ld.generate_batch(b, **dict(dict(ddim_steps=4, unconditional_guidance_scale=3.5), **kw)),
            "generate_batch_masked": lambda b, **kw: ld.generate_batch_masked(b, **dict(dict(ddim_steps=4,
                                                                                          unconditional_guidance_scale=3.5), **kw)),
            "generate_batch_from_audio": lambda b, **kw: ld.generate_batch_from_audio(b, 0.5, **dict(
                dict(ddim_steps=4, unconditional_guidance_scale=3.5), **kw)),
            "generate_batch_long": lambda b, **kw: ld.generate_batch_long(b, 768, **dict(dict(ddim_steps=4,
                                                                                           unconditional_guidance_scale=3.5), **kw)),
            "generate_batch_long_from_audio": lambda b, **kw: ld.generate_batch_long_from_audio(
                b, 768, [(0, 200)], **dict(dict(ddim_steps=4, unconditional_guidance_scale=3.5), **kw))}
    for name, job in jobs.items():
        long_form = "long" in name
        cases = [((batches, dict(weights=w, n_gen=2)), "n_gen"), ((batches, dict(weights=w[:2])), r"shape \[3\]"),
                 ((batches, dict(weights=[1.0, float("nan"), 0.5])), "finite"), ((batches, dict(weights=[0.0, 0.0, 0.0])), "every weight is 0"),
                 ((batches, dict(weights=[[1.0, 0.5, 0.2]] * 3)), "3 entries for ddim_steps=4"),
                 ((batches, dict(weights=w, unconditional_guidance_scale=1.0)), "unconditional conditioning"),
                 ((batches[0], dict(weights=[1.0])), "list of batches"), (([], dict(weights=[])), "list of batches"),
                 ((batches * 3, dict(weights=w * 3)), "at most 8"),
                 (([batches[0], make_batch_for_text_to_audio("x", batchsize=2)], dict(weights=[1.0, 0.5])), "one size")]
        if name != "generate_batch_from_audio":
            cases.append(((batches, dict(weights=w, shard=(0, 2))), "shard"))
        if long_form:
            cases.append(((batches, dict(weights=w, boundaries=[300.0, 500.0])), "timeline"))
        else:
            cases.append(((batches, dict(weights=w, ddim_steps=None)), "ddim_steps"))
        for (b, kw), msg in cases:
            with pytest.raises(ValueError, match=msg):
                job(b, **kw)
    assert torch.equal(torch.get_rng_state(), state)         # nothing was drawn


def test_compose_entries_weights_and_schedules():
    from audioldm2_amd.pipeline import compose_entries
    ld = _NoGpu()
    prompts, trans, w = compose_entries(MIX, 200, ld)
    assert prompts == [p for p, _ in MIX] and trans == ["", "", ""] and w.dtype == np.float64 and w.tolist() == [1.0, 0.6, -0.4]
    # a transcription rides on an entry; an integer weight is a number
    prompts, trans, w = compose_entries([("a voice", 1, "hello there"), ("wind", 0.5)], None, ld)
    assert trans == ["hello there", ""] and w.tolist() == [1.0, 0.5]
    # one listed weight makes a schedule: the scalar is repeated, sampler order (the noisiest step first)
    fade = [1.0, 0.75, 0.5, 0.25]
    _, _, w = compose_entries([("rain", 1.0), ("thunder", fade)], 4, ld)
    assert w.shape == (4, 2) and w[:, 0].tolist() == [1.0] * 4 and w[:, 1].tolist() == fade
    # ddim_steps = 6 does not divide 1000: the reference's grid has 7 entries, the last weight is repeated for the extra step
    _, _, w = compose_entries([("rain", [0.1 * i for i in range(1, 7)])], 6, ld)
    assert w.shape == (7, 1) and w[-1, 0] == w[-2, 0] == pytest.approx(0.6)


def test_signatures_carry_the_keyword():
    import audioldm2_amd.pipeline as P
    for f in (P.text_to_audio, P.text_to_audio_long, P.extend_audio):
        assert inspect.signature(f).parameters["compose"].default is None
    assert list(inspect.signature(P.text_to_audio).parameters)[-1] == "sampler"        # `sampler` stays the last parameter
    # audio_to_audio's parameter list is pinned (tests/test_audio2audio_cpu.py): its composed jobs take the method's `weights=`
    assert "compose" not in inspect.signature(P.audio_to_audio).parameters
    for f in (P.LatentDiffusion.generate_batch_long, P.LatentDiffusion.generate_batch_long_from_audio):
        assert inspect.signature(f).parameters["weights"].default is None
