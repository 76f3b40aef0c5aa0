"""Test-only harness for the denoise engine's state machine: the tiny models (SD1.5 UNet, two ControlNets, SDXL UNet), their
fp32 oracles and fp16 arms built once; a generation as a small frozen ``Spec``; the inputs, the pipeline call, a fresh eager
run and the oracle pair of a spec, each memoised per spec and left unchanged; ``Gen`` and ``run_scenario``, which run a
list of specs on one live pipeline and hold every generation to the fresh eager bits, the oracle and the capture count.
tests/test_gpu_engine_reuse.py and tests/test_gpu_engine_features.py are lists of such scenarios;
tests/test_gpu_multicontrolnet.py takes its models and loop inputs from here.

A spec with ``scheduler="lcm"`` runs LCMScheduler with the noise of its inputs; at guidance_scale <= 1, or on the UNet with
``time_cond_proj_dim`` (``time_cond``), the engine takes the single pass (``single_pass``): the oracle then sees the conditional
rows only (lcm_ref.CondOnly), and ``run_scenario`` holds the step launch and the UNet's batch rows of every generation.

FreeU and community LoRAs are state of the UNet, not arguments of a call: ``apply_features`` brings a live pipeline from the
state its UNet is in to the one a spec names, and calls nothing where they agree."""
import functools
import weakref
from dataclasses import dataclass, fields, replace
from typing import Any, Callable, Optional, Tuple

import torch

from conftest import check_vs_fp16_arm, dev_half, half_arm
from oracle_utils import build_oracle, make_weights, product_cfg

NET_SEEDS = {"A": 3, "B": 4}        # the two tiny ControlNets
ADAPTER_SEEDS = (1, 7)              # adapter 0: what make_weights gives the UNet; adapter 1: a second synthetic checkpoint


# --------------------------------------------------------------------------- models (built once)
@functools.lru_cache(maxsize=None)
def models(dev_str):
    from consistentid_amd import synth
    from consistentid_amd.controlnet import HipControlNet
    from consistentid_amd.unet import HipUNet
    from oracle import unet as ounet
    from oracle.controlnet import ControlNetModel
    dev = torch.device(dev_str)
    cfg = product_cfg("tiny")
    o_cns, sds = [], []
    for seed in NET_SEEDS.values():
        sd = synth.random_controlnet_state_dict(cfg, seed=seed)
        o = ControlNetModel(ounet.tiny_config("sd15"))
        o.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
        o_cns.append(o.eval())
        sds.append(sd)
    _, sd, ad = make_weights("tiny", rank=8)
    o_unet = build_oracle("tiny", sd, ad, rank=8)
    return dict(cfg=cfg, o_cns=o_cns, cn_sds=sds, o_unet=o_unet, unet_sd=(sd, ad),
                a_cns=[half_arm(o, dev) for o in o_cns], a_unet=half_arm(o_unet, dev),
                new_cn=lambda k: HipControlNet(cfg, sds[k], device=dev), new_unet=lambda: HipUNet(cfg, sd, ad, device=dev))


def loop_inputs(cfg, B=2):
    from consistentid_amd import synth
    side = cfg.sample_size * 8
    inp = synth.random_inputs(cfg, B, side, side)
    gen = torch.Generator().manual_seed(21)
    imgs = [torch.rand(B, 3, side, side, generator=gen).half() for _ in range(2)]
    init = torch.randn(B, 4, side // 8, side // 8, generator=gen).half()
    noise = torch.randn(B, 4, side // 8, side // 8, generator=gen).half()
    mask = (torch.rand(B, 1, side // 8, side // 8, generator=gen) > 0.5).half()
    return inp, imgs, init, noise, mask


class OracleMulti:
    """What the reference's loop does around ``self.controlnet(...)`` with a MultiControlNetModel, for oracle.loop.denoise:
    counts its calls (= the step index), applies scale_k * keep_k[i] itself (CN :363-370, :397-398) and sums the nets'
    residuals as diffusers does.  The loop's own window stays (0, 1) and its scale 1."""

    def __init__(self, nets, scales, windows, n_steps):
        self.nets, self.scales, self.calls = nets, scales, 0
        self.keep = [[1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in windows] for i in range(n_steps)]

    def __call__(self, sample, t, cond, control_images, conditioning_scale=1.0):
        assert conditioning_scale == 1.0
        i, self.calls = self.calls, self.calls + 1
        down = mid = None
        for k, net in enumerate(self.nets):
            d, m = net(sample, t, cond, control_images[k], conditioning_scale=self.scales[k] * self.keep[i][k])
            down, mid = (d, m) if down is None else ([a + b for a, b in zip(down, d)], mid + m)
        return down, mid


@functools.lru_cache(maxsize=None)
def unet_models(dev_str, name="tiny", adapter=0):
    """(cfg, unet state dict, adapter dict, fp32 oracle, fp16 arm) of the tiny SD1.5 / SDXL UNet with adapter 0 or 1 merged"""
    from consistentid_amd import synth
    if name == "tiny" and adapter == 0:
        M = models(dev_str)
        return M["cfg"], *M["unet_sd"], M["o_unet"], M["a_unet"]
    cfg, sd, ad = make_weights(name, rank=8)
    if adapter:
        ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=ADAPTER_SEEDS[adapter])
    oracle = build_oracle(name, sd, ad, rank=8)
    return cfg, sd, ad, oracle, half_arm(oracle, torch.device(dev_str))


def new_unet(dev_str, name="tiny", adapter=0, keep_base=False, time_cond=False):
    from consistentid_amd.unet import HipUNet
    if time_cond:
        assert (name, adapter) == ("tiny", 0)
        C = time_cond_models(dev_str)
        return HipUNet(C["cfg"], C["sd"], C["ad"], device=torch.device(dev_str), keep_base=keep_base)
    cfg, sd, ad, _, _ = unet_models(dev_str, name, adapter)
    return HipUNet(cfg, sd, ad, device=torch.device(dev_str), keep_base=keep_base)


def new_net(dev_str, label):
    return models(dev_str)["new_cn"](list(NET_SEEDS).index(label))


# --------------------------------------------------------------------------- a UNet with time_cond_proj_dim
COND_DIM = 32
_COND = {}


def time_cond_models(dev):
    """tiny SD1.5 UNet with time_cond_proj_dim = 32: (cfg, state dict, HipUNet, (fp32 oracle, fp16 arm), the guidance holder).
    The oracle UNet has no cond_proj: a forward pre-hook on its time_embedding adds cond_proj(w_emb) to the sinusoid rows,
    computed here in fp32 from the fp16 embedding the UNet is handed.  One set per device (``hip`` on a GPU only): the oracle
    pair reads the guidance row from ``holder``, which ``set_guidance`` fills before a run."""
    dev = torch.device(dev)
    if str(dev) not in _COND:
        cfg, sd, ad = make_weights("tiny", rank=8, time_cond_proj_dim=COND_DIM)
        w_cond = sd["time_embedding.cond_proj.weight"].half().float()
        assert tuple(w_cond.shape) == (cfg.block_out_channels[0], COND_DIM)
        oracle = build_oracle("tiny", {k: v for k, v in sd.items() if k != "time_embedding.cond_proj.weight"}, ad, rank=8)
        holder = {}

        def add_cond(mod, args):
            return (args[0] + holder["row"].to(args[0]),)
        oracle.time_embedding.register_forward_pre_hook(add_cond)
        C = dict(cfg=cfg, sd=sd, ad=ad, w_cond=w_cond, holder=holder, oracles=(oracle, half_arm(oracle, dev)))
        if dev.type == "cuda":
            from consistentid_amd.unet import HipUNet
            C["hip"] = HipUNet(cfg, sd, ad, device=dev)
        _COND[str(dev)] = C
    return _COND[str(dev)]


def set_guidance(C, guidance):
    from lcm_ref import guidance_scale_embedding
    w_emb = torch.from_numpy(guidance_scale_embedding(guidance - 1.0, COND_DIM)).half().float()
    C["holder"]["row"] = (w_emb @ C["w_cond"].T)[None]
    return w_emb


# --------------------------------------------------------------------------- a generation
@dataclass(frozen=True)
class Spec:
    pipe: str = "txt2img"                       # "txt2img" | "inpaint" | "controlnet" (SD1.5 tiny) | "sdxl" (SDXL tiny)
    scheduler: str = "ddim"                     # "ddim" | "euler" | "dpm" | "pndm" | "lcm"
    steps: int = 4                              # num_inference_steps
    guidance: float = 5.0
    merge: int = 1                              # start_merge_step
    strength: float = 1.0                       # inpaint pipelines
    B: int = 2
    hw: Optional[Tuple[int, int]] = None        # latent size; None: sample_size x sample_size
    text_len: int = 77
    seed: int = 0                               # of every input value
    nets: Tuple[str, ...] = ()                  # "controlnet": labels of NET_SEEDS, in the order they run
    multi: bool = False                         # a HipMultiControlNet of ``nets`` (a plain net otherwise)
    scales: Tuple[float, ...] = ()              # per net, in the order of ``nets``
    windows: Tuple[Tuple[float, float], ...] = ()
    eta: float = 0.0                            # > 0: DDIM with given variance_noise (drawn from ``seed``)
    callback: bool = False
    adapter: int = 0                            # which adapter the UNet has merged
    null_post: bool = False                     # "sdxl": a second unconditional set after the merge
    time_ids: Tuple[int, int] = (0, 0)          # "sdxl": crop offsets in add_time_ids
    freeu: Optional[Tuple[float, float, float, float]] = None       # (s1, s2, b1, b2) of enable_freeu; None: disabled
    rescale: float = 0.0                        # guidance_rescale
    prediction: str = "epsilon"                 # the scheduler's prediction_type: "epsilon" | "v_prediction"
    zero_snr: bool = False                      # DDIM with test_gpu_guidance_rescale.ZERO_SNR (needs "v_prediction")
    loras: Tuple[Tuple[int, float], ...] = ()   # (seed of lora_cases.unet_lora, adapter weight), in load order
    time_cond: bool = False                     # the tiny SD1.5 UNet with time_cond_proj_dim = 32 (``time_cond_models``; needs "lcm")
    # (key of PAG_SELECTIONS, pag_scale, pag_adaptive_scale); a scale of 0: the layers are selected and the call is a plain one
    pag: Optional[Tuple[str, float, float]] = None
    sag: float = 0.0                            # sag_scale

    def __post_init__(self):
        """what the engine refuses is no spec: ``refused`` names it for the tests of the refusals"""
        why = refused(self)
        if why:
            raise ValueError(f"{why} is refused by the engine: no generation to describe")

    def but(self, **kw):
        return replace(self, **kw)

    @property
    def name(self):
        return "tinyxl" if self.pipe == "sdxl" else "tiny"


def pag_on(spec):
    return spec.pag is not None and spec.pag[1] > 0.0


def refused(spec):
    """the combination in ``spec`` that DenoiseEngine.run answers with NotImplementedError, or None"""
    if pag_on(spec) and spec.sag > 0.0:
        return "PAG together with SAG"
    for name, on in (("PAG", pag_on(spec)), ("SAG", spec.sag > 0.0)):
        if on and spec.rescale > 0.0:
            return f"{name} together with guidance_rescale"
        if on and spec.nets:
            return f"{name} with ControlNets"
    return None


# per model: selection key -> (the ids enable_pag is given, the oracle's module paths)
PAG_SELECTIONS = {
    "tiny": {"mid": ("mid", ("mid_block",)), "first-down": ("down.block_0", ("down_blocks.0",)),
             "all": (["down.block_0", "down.block_1", "mid", "up.block_1", "up.block_2"], ("down_blocks", "mid_block", "up_blocks"))},
    "tinyxl": {"mid": ("mid", ("mid_block",)), "first-down": ("down.block_1", ("down_blocks.1",)),
               "all": (["down.block_1", "mid", "up.block_0"], ("down_blocks", "mid_block", "up_blocks"))}}


def pipeline_class(spec):
    from consistentid_amd import pipeline
    return {"txt2img": pipeline.ConsistentIDStableDiffusionPipeline, "sdxl": pipeline.ConsistentIDStableDiffusionXLPipeline,
            "inpaint": pipeline.StableDiffusionInpaintConsistentIDPipeline,
            "controlnet": pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline}[spec.pipe]


def scheduler_kwargs(spec):
    """the constructor arguments both the product's scheduler and its restatement take: none for an all-default spec"""
    kw = {}
    if spec.prediction != "epsilon":
        kw["prediction_type"] = spec.prediction
    if spec.zero_snr:
        from test_gpu_guidance_rescale import ZERO_SNR
        assert spec.scheduler == "ddim", "rescale_betas_zero_snr is DDIMScheduler's"
        kw.update(ZERO_SNR)
    return kw


def product_scheduler(spec):
    from consistentid_amd import scheduler
    return {"ddim": scheduler.DDIMScheduler, "euler": scheduler.EulerDiscreteScheduler, "lcm": scheduler.LCMScheduler,
            "dpm": scheduler.DPMSolverMultistepScheduler, "pndm": scheduler.PNDMScheduler}[spec.scheduler](**scheduler_kwargs(spec))


def single_pass(spec):
    """whether the engine runs the B conditional rows only: LCMScheduler at guidance_scale <= 1, or on the
    UNet with time_cond_proj_dim"""
    assert not spec.time_cond or (spec.scheduler == "lcm" and spec.pipe != "sdxl" and not spec.adapter and not spec.loras)
    return spec.scheduler == "lcm" and (spec.time_cond or spec.guidance <= 1.0)


def expected_step_path(spec):
    """the step launch the engine must report: the single-pass kernel; else the first-order CFG kernel for DDIM at eta 0 and
    Euler, the multistep CFG kernel for the others, ``+rescale`` where guidance_rescale is honoured; ``+pag`` / ``+sag`` behind
    either under a guidance"""
    guided = "+pag" if pag_on(spec) else "+sag" if spec.sag > 0.0 else ""
    if single_pass(spec):
        return "multistep" + guided
    first_order = spec.scheduler in ("ddim", "euler") and spec.eta == 0.0
    return ("cfg_ddim" if first_order else "cfg_multistep") + ("+rescale" if spec.rescale > 0.0 and spec.guidance > 1.0 else "") + guided


def mid_size(spec):
    """(H_mid, W_mid): every down block but the last halves the latent size"""
    cfg = product_cfg(spec.name)
    h, w = spec.hw or (cfg.sample_size, cfg.sample_size)
    for _ in range(len(cfg.block_out_channels) - 1):
        h, w = h // 2, w // 2
    return h, w


def unet_rows(spec):
    """the UNet's batch rows in a step: [uncond |] cond [| perturbed]"""
    return ((1 if single_pass(spec) else 2) + pag_on(spec)) * spec.B


def scheduler_key(spec):
    """what ``pipe.scheduler`` has to be rebuilt for"""
    return spec.scheduler, spec.prediction, spec.zero_snr


def active_sets(spec):
    """{tuple of the indices of the nets that run: number of executed steps it runs in} (() where no net runs), from the
    product's own keep table"""
    from collections import Counter
    from consistentid_amd.controlnet import active_nets, controlnet_keep_table
    n = executed_steps(spec)                # (the engine's windows count schedule entries, PNDM's doubled first step included)
    if not spec.nets:
        return {(): n}
    return dict(Counter(active_nets(row) for row in controlnet_keep_table(n, [w[0] for w in spec.windows], [w[1] for w in spec.windows])))


def executed_steps(spec):
    """UNet evaluations of the generation (PNDM's first step takes two)"""
    n = spec.steps + (spec.scheduler == "pndm")
    return n if spec.strength == 1.0 else min(int(spec.steps * spec.strength), spec.steps)


def inputs(spec, dev_str):
    """every input value of a generation, on the CPU in fp16 (fp16-representable: the oracle sees the same numbers); they depend
    on the shapes and the seed only, so two specs that differ in anything else share the very same tensors"""
    return _inputs(spec.name, spec.B, spec.hw, spec.text_len, spec.seed, executed_steps(spec), spec.time_ids, dev_str)


@functools.lru_cache(maxsize=None)
def _inputs(name, B, hw, text_len, seed, n_run, time_ids, dev_str):
    from consistentid_amd import synth
    cfg = unet_models(dev_str, name)[0]
    h, w = hw or (cfg.sample_size, cfg.sample_size)
    inp = synth.random_inputs(cfg, B, 8 * h, 8 * w, seed_latents=2024 + seed, seed_embeds=1 + seed, text_len=text_len)
    gen = torch.Generator().manual_seed(21 + seed)
    lshape = (B, 4, h, w)
    inp["imgs"] = {k: torch.rand(B, 3, 8 * h, 8 * w, generator=gen).half() for k in NET_SEEDS}
    inp["init"], inp["noise"] = torch.randn(lshape, generator=gen).half(), torch.randn(lshape, generator=gen).half()
    inp["mask"] = (torch.rand(B, 1, h, w, generator=gen) > 0.5).half()
    inp["null_post"] = (inp["null"].float() + 0.5 * torch.randn(inp["null"].shape, generator=gen)).half()
    inp["variance_noise"] = torch.randn(n_run, *lshape, generator=gen).half()
    if "time_ids" in inp:
        inp["time_ids"][:, 2], inp["time_ids"][:, 3] = time_ids
    return inp


def call_pipeline(pipe, spec, dev, extra=None, on_step=None):
    """one generation of ``spec`` on ``pipe`` (whose controlnet attribute is already the spec's) -> (latents, [per-step clones]);
    ``extra``: further keywords of the call (a scale of 0.0 spelled out, which a spec cannot say); ``on_step(i)``: called after
    executed step i, between the launches (it may look at the engine; the latents are not its business)"""
    inp = inputs(spec, str(dev))
    d = lambda t: t.to(dev)
    steps = []
    kw = dict(prompt_embeds=d(torch.cat([inp["null"], inp["augmented"], inp["text"]])), latents=d(inp["latents"]),
              num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge, output_type="latent")
    if spec.callback and on_step is None:
        kw["callback"] = lambda i, t, lat: steps.append(lat.clone())
    elif on_step is not None:
        kw["callback"] = lambda i, t, lat: (steps.append(lat.clone()) if spec.callback else None, on_step(i))
    if spec.eta > 0.0:
        kw.update(eta=spec.eta, variance_noise=d(inp["variance_noise"]))
    if spec.scheduler == "lcm" and executed_steps(spec) > 1:    # one tensor per executed step but the last; one step: none
        kw["variance_noise"] = d(inp["variance_noise"][:executed_steps(spec) - 1])
    if spec.rescale > 0.0:
        kw["guidance_rescale"] = spec.rescale
    if spec.pipe in ("inpaint", "controlnet"):
        kw.update(image_latents=d(inp["init"]), noise=d(inp["noise"]), mask_latents=d(inp["mask"]), strength=spec.strength)
    if spec.pipe == "controlnet" and spec.nets:
        imgs = [d(inp["imgs"][k]) for k in spec.nets]
        starts, ends = [w[0] for w in spec.windows], [w[1] for w in spec.windows]
        if spec.multi:
            kw.update(control_image=imgs, controlnet_conditioning_scale=list(spec.scales), control_guidance_start=starts,
                      control_guidance_end=ends)
        else:
            kw.update(control_image=imgs[0], controlnet_conditioning_scale=spec.scales[0], control_guidance_start=starts[0],
                      control_guidance_end=ends[0])
    if spec.pipe == "sdxl":
        kw.update(pooled_prompt_embeds=inp["pooled_augmented"], pooled_prompt_embeds_text_only=inp["pooled_text"],
                  negative_pooled_prompt_embeds=inp["pooled_null"], add_time_ids=inp["time_ids"])
        if spec.null_post:
            kw["negative_prompt_embeds_facial"] = d(inp["null_post"])
    if pag_on(spec):
        kw.update(pag_scale=spec.pag[1], pag_adaptive_scale=spec.pag[2])
    if spec.sag > 0.0:
        kw["sag_scale"] = spec.sag
    out = pipe(**kw, **(extra or {})).images
    torch.cuda.synchronize()
    return out, steps


# --------------------------------------------------------------------------- FreeU and LoRA: state of the UNet
@functools.lru_cache(maxsize=None)
def lora_file(name, seed):
    """``lora_cases.unet_lora(name, seed)`` as a kohya file of its family: SD1.5 with proj_in / proj_out shaped like 1x1
    convolutions, SDXL with SGM names (what tests/test_gpu_lora.py loads)"""
    import lora_cases as L
    from consistentid_amd import lora
    modules = L.unet_lora(name, seed=seed)
    if name == "tinyxl":
        cfg = product_cfg(name)
        return L.to_kohya(modules, name_of=lambda p: lora.sgm_path(cfg, p))
    return L.to_kohya(modules, conv=True)


# UNet -> (the loras of the last spec applied to it, a weak reference to the pipeline that loaded them): the adapters are held
# by a pipeline but merged into the UNet, which several pipelines may share
_LORA_STATE = weakref.WeakKeyDictionary()


# UNet -> the key of PAG_SELECTIONS that enable_pag was last given through ``apply_features``
_PAG_STATE = weakref.WeakKeyDictionary()


def apply_features(pipe, spec):
    """bring ``pipe``'s UNet from the FreeU / LoRA / PAG-selection state it is in to ``spec``'s, through ``pipe``'s own
    diffusers-style methods and only where the state differs: enable_freeu / disable_freeu, unload_lora_weights (on the
    pipeline that loaded) / load_lora_weights / set_adapters, and enable_pag / disable_pag.  -> whether anything was called"""
    unet, name = pipe.unet, spec.name
    called = False
    key = spec.pag[0] if spec.pag is not None else None
    if _PAG_STATE.get(unet) != key:
        if key is None:
            pipe.disable_pag()
        else:
            pipe.enable_pag(PAG_SELECTIONS[name][key][0])
        _PAG_STATE[unet] = key
        called = True
    assert bool(unet.pag_layers) == (key is not None)
    if unet._freeu != spec.freeu:
        if spec.freeu is None:
            pipe.disable_freeu()
        else:
            pipe.enable_freeu(*spec.freeu)
        called = True
    assert unet._freeu == spec.freeu
    loaded, holder = _LORA_STATE.get(unet, ((), None))
    if loaded != spec.loras:
        if loaded:
            holder().unload_lora_weights()
        for seed, _ in spec.loras:
            pipe.load_lora_weights(lora_file(name, seed), adapter_name=f"seed{seed}")
        if any(w != 1.0 for _, w in spec.loras):
            pipe.set_adapters([f"seed{seed}" for seed, _ in spec.loras], [w for _, w in spec.loras])
        _LORA_STATE[unet] = (spec.loras, weakref.ref(pipe) if spec.loras else None)
        called = True
    return called


def controlnet_of(spec, net_objects):
    """the pipeline's ``controlnet`` for ``spec`` out of {label: HipControlNet}"""
    from consistentid_amd.controlnet import HipMultiControlNet
    if not spec.nets:
        return None
    return HipMultiControlNet([net_objects[k] for k in spec.nets]) if spec.multi else net_objects[spec.nets[0]]


@functools.lru_cache(maxsize=None)
def fresh_eager(spec, dev_str):
    """``spec`` on objects nothing else has touched: a new HipUNet (with ``keep_base`` where a LoRA is to be merged), new
    HipControlNets from the same state dicts, a new pipeline with use_graph=False brought to the spec's FreeU / LoRA state
    -> (latents, [per-step clones])"""
    dev = torch.device(dev_str)
    kw = {}
    if spec.pipe == "controlnet":
        kw["controlnet"] = controlnet_of(spec, {k: new_net(dev_str, k) for k in spec.nets})
    unet = new_unet(dev_str, spec.name, spec.adapter, keep_base=bool(spec.loras) or spec.pag is not None, time_cond=spec.time_cond)
    pipe = pipeline_class(spec)(unet, scheduler=product_scheduler(spec), use_graph=False, **kw)
    apply_features(pipe, spec)
    out, steps = call_pipeline(pipe, spec, dev)
    assert not pipe._engine.captures
    return out.clone(), steps


# --------------------------------------------------------------------------- the oracle of a spec
@functools.lru_cache(maxsize=None)
def oracle_models(dev_str, name="tiny", adapter=0, loras=(), time_cond=False):
    """(fp32 oracle, fp16 arm) of the UNet with the LoRAs of ``loras`` merged in float64 (lora_cases.merged_state_dict);
    ``loras`` = (): the pair of ``unet_models``.  ``time_cond``: the hooked pair of ``time_cond_models``"""
    if time_cond:
        assert (name, adapter, loras) == ("tiny", 0, ())
        return time_cond_models(dev_str)["oracles"]
    _, sd, ad, oracle, arm = unet_models(dev_str, name, adapter)
    if not loras:
        return oracle, arm
    import lora_cases as L
    merged = build_oracle(name, L.merged_state_dict(sd, [(L.unet_lora(name, seed=seed), w) for seed, w in loras]), ad, rank=8)
    return merged, half_arm(merged, torch.device(dev_str))


def reference_scheduler(spec, noises):
    """the stateful restatement ``oracle.loop.denoise`` steps with, timesteps set: tests/multistep_ref.py and oracle/ddim.py
    as before for an epsilon-prediction spec, tests/vpred_ref.py wherever ``prediction`` or ``zero_snr`` is set,
    tests/lcm_ref.py for "lcm"."""
    from lcm_ref import LCMLoopRef
    from multistep_ref import DDIMEtaRef, DPMSolverPP2MRef, PNDMRef
    from oracle import ddim
    kw = scheduler_kwargs(spec)
    if spec.eta > 0.0:
        assert spec.scheduler == "ddim"
    if spec.scheduler == "lcm":         # tests/lcm_ref.py: the noises of the executed steps but the last, in call order
        sch = LCMLoopRef(noises[:executed_steps(spec) - 1], **kw)
    elif kw:
        from vpred_ref import DDIMRef, DPMSolverVRef, EulerRef, PNDMVRef
        if spec.scheduler == "ddim":
            sch = DDIMRef(eta=spec.eta, noises=noises if spec.eta > 0.0 else (), **kw)
        else:
            sch = {"euler": EulerRef, "dpm": DPMSolverVRef, "pndm": PNDMVRef}[spec.scheduler](**kw)
    elif spec.eta > 0.0:
        return DDIMEtaRef(spec.eta, noises)
    else:
        sch = {"ddim": ddim.DDIMScheduler, "euler": ddim.EulerDiscreteScheduler, "dpm": DPMSolverPP2MRef, "pndm": PNDMRef}[spec.scheduler]()
    sch.set_timesteps(spec.steps)       # the pipelines set the timesteps before scaling the initial noise (ref :510, :517)
    return sch


def oracle_run(spec, dev_str, arm=False, misindexed=False):
    """the latents of ``oracle_traced`` (which is memoised)"""
    return oracle_traced(spec, dev_str, arm, misindexed)[0]


def guidance_trace(spec, dev_str, arm=False, misindexed=False):
    """what the guided oracle UNet recorded while ``spec`` ran: (SAG: column masses per evaluation, masks per evaluation; PAG:
    (s_i, |c - p| / |c|) per step)"""
    return oracle_traced(spec.but(callback=False), dev_str, arm, misindexed)[1]


@functools.lru_cache(maxsize=None)
def oracle_traced(spec, dev_str, arm=False, misindexed=False):
    """-> (latents, (masses, masks, seen) of the guided UNet, empty without a guidance).  ``spec`` through ``oracle.loop.denoise``, unchanged: on the fp32 oracle on the CPU (needs no GPU), or with ``arm`` on its
    fp16 copy on ``dev_str``.  LoRAs are merged into the oracle's state dict; guidance_rescale wraps the UNet
    (vpred_ref.RescaledUNet); FreeU hooks the UNet's first two up blocks (freeu_ref.install_freeu) for this call only -- the
    models are memoised and shared with other modules, so the handles are removed before this returns.  Where the engine
    takes the single pass (``single_pass``) the UNet sits behind lcm_ref.CondOnly -- the loop's u + g (c - u) is then exactly c
    -- and guidance_rescale is inert, as in the product; the time-cond pair gets its guidance row first.  PAG / SAG put
    ``guided_unet`` in front (which evaluates the conditional rows only by itself in the single pass)."""
    from freeu_ref import install_freeu
    from lcm_ref import CondOnly
    from oracle import loop
    from vpred_ref import RescaledUNet
    single = single_pass(spec)
    if single and spec.rescale > 0.0:
        return oracle_traced(spec.but(rescale=0.0), dev_str, arm, misindexed)
    dev = torch.device(dev_str)
    M = models(dev_str)
    unet = oracle_models(dev_str, spec.name, spec.adapter, spec.loras, spec.time_cond)[int(arm)]
    if spec.time_cond:
        set_guidance(time_cond_models(dev_str), spec.guidance)
    pool = M["a_cns" if arm else "o_cns"]
    nets = [pool[list(NET_SEEDS).index(k)] for k in spec.nets]
    f = (lambda t: dev_half(t, dev)) if arm else (lambda t: t.float())
    inp = inputs(spec, dev_str)
    sch = reference_scheduler(spec, list(inp["variance_noise"].float()))
    kw = dict(num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge)
    if spec.pipe in ("inpaint", "controlnet"):
        kw.update(inpaint_mask=f(inp["mask"]), inpaint_init=f(inp["init"]), inpaint_noise=f(inp["noise"]), strength=spec.strength)
    if spec.pipe == "sdxl":
        kw.update(add_text_embeds_null=f(inp["pooled_null"]), add_text_embeds_text=f(inp["pooled_text"]),
                  add_text_embeds_aug=f(inp["pooled_augmented"]), add_time_ids=f(inp["time_ids"]))
        if spec.null_post:
            kw["null_embeds_post"] = f(inp["null_post"])
    wrap = None
    if nets and spec.multi:
        wrap = OracleMulti(nets, list(spec.scales), list(spec.windows), executed_steps(spec))
        kw.update(controlnet=wrap, control_image=[f(inp["imgs"][k]) for k in spec.nets])
    elif nets:
        kw.update(controlnet=nets[0], control_image=f(inp["imgs"][spec.nets[0]]), conditioning_scale=spec.scales[0],
                  control_guidance_start=spec.windows[0][0], control_guidance_end=spec.windows[0][1])
    handles = install_freeu(unet, *spec.freeu) if spec.freeu is not None else []
    try:
        model = RescaledUNet(unet, spec.guidance, spec.rescale) if spec.rescale > 0.0 and spec.guidance > 1.0 else unet
        model = CondOnly(model) if single else model
        if pag_on(spec) or spec.sag > 0.0:          # (neither goes with guidance_rescale or nets: ``refused``)
            model = guided_unet(spec, unet, sch, misindexed)
        out = loop.denoise(model, sch, f(inp["latents"]) * float(sch.init_noise_sigma), f(inp["null"]), f(inp["augmented"]),
                           f(inp["text"]), **kw)
    finally:
        for h in handles:
            h.remove()
    assert wrap is None or wrap.calls == executed_steps(spec)
    return out, (tuple(getattr(model, "masses", ())), tuple(getattr(model, "masks", ())), tuple(getattr(model, "seen", ())))


class _EarlierTimestep:
    """a reference scheduler whose noise model is read ``shift`` schedule entries early: what a per-step column gives when it
    is indexed by the executed step, not by the schedule entry, in a generation that starts at entry ``shift``"""

    def __init__(self, sch, shift):
        self.sch, self.shift = sch, shift

    def _t(self, t):
        ts = [int(v) for v in self.sch.timesteps]
        return self.sch.timesteps[ts.index(int(t)) - self.shift]

    def add_noise(self, a, b, t):
        return self.sch.add_noise(a, b, self._t(t))

    def scale_model_input(self, x, t):
        return self.sch.scale_model_input(x, self._t(t))


def first_step(spec):
    """the schedule entry the generation starts at (strength < 1)"""
    return spec.steps + (spec.scheduler == "pndm") - executed_steps(spec)


def guided_unet(spec, unet, sch, misindexed=False):
    """pag_ref.PagUNet / sag_ref.SagUNet in front of ``unet``, as tests/test_gpu_pag.py and tests/test_gpu_sag.py put them.
    ``misindexed``: the PAG scale / SAG's noise model of the schedule entry ``first_step`` entries early -- the reference of
    the mistake, for the assertion that a generation at strength < 1 can tell the two apart"""
    import pag_ref
    import sag_ref
    single, shift = single_pass(spec), first_step(spec) if misindexed else 0
    assert not misindexed or shift > 0
    if spec.sag > 0.0:
        return sag_ref.SagUNet(unet, _EarlierTimestep(sch, shift) if shift else sch, spec.guidance, spec.sag, single=single,
                               prediction=spec.prediction)
    _, scale, adaptive = spec.pag
    model = pag_ref.PagUNet(unet, PAG_SELECTIONS[spec.name][spec.pag[0]][1], spec.guidance, scale, adaptive, single=single)
    return _EarlierPagScale(model, [int(v) for v in sch.timesteps], shift) if shift else model


class _EarlierPagScale:
    """``pag_ref.PagUNet`` handed the scale of the schedule entry ``shift`` entries early (see ``_EarlierTimestep``)"""

    def __init__(self, model, ts, shift):
        self.model, self.ts, self.shift, self.scales = model, ts, shift, (model.pag_scale, model.adaptive)

    @property
    def seen(self):
        return self.model.seen

    def __call__(self, sample, t, *a, **kw):
        import pag_ref
        self.model.pag_scale, self.model.adaptive = pag_ref.scale_at(*self.scales, self.ts[self.ts.index(int(t)) - self.shift]), 0.0
        return self.model(sample, t, *a, **kw)


def oracle_pair(spec, dev_str):
    """(fp32 oracle latents, fp16-arm latents) of ``spec``"""
    return oracle_run(spec, dev_str), oracle_run(spec, dev_str, True)


def hooked_modules(*roots):
    """the submodules of ``roots`` that carry a forward pre-hook: none, unless ``oracle_run`` left FreeU installed"""
    return [m for root in roots for m in root.modules() if m._forward_pre_hooks]


FEATURES = ("freeu", "rescale", "loras", "pag", "sag")      # the fields a spec can switch on that the engine could silently ignore


def features_on(spec):
    """(guidance_rescale is inert in the single pass: it is no feature of such a spec)"""
    return [k for k in FEATURES if getattr(spec, k) != getattr(Spec(), k) and not (k == "rescale" and single_pass(spec))
            and not (k == "pag" and not pag_on(spec))]


@functools.lru_cache(maxsize=None)
def features_moved(spec, dev_str="cpu"):
    """{feature that ``spec`` switches on: relative L2 distance, on the fp32 oracle alone, between ``spec`` and the same spec
    with only that feature off}.  A parity test of ``spec`` says something about the feature only where this is far above
    the parity tolerance (``assert_features_matter``)."""
    from conftest import rel_l2
    spec = spec.but(callback=False)
    return {k: rel_l2(oracle_run(spec, dev_str), oracle_run(spec.but(**{k: getattr(Spec(), k)}), dev_str)) for k in features_on(spec)}


def assert_misindexed_differs(spec, dev_str="cpu"):
    """on the fp32 oracle: ``spec`` (strength < 1) and the same generation with the guidance's per-step column read at the
    executed step are 20 * TOL_L2 apart, so the comparison with the oracle tells the two indexings apart"""
    from conftest import TOL_L2, rel_l2
    spec = spec.but(callback=False)
    assert first_step(spec) > 0 and (pag_on(spec) or spec.sag > 0.0), spec
    apart = rel_l2(oracle_run(spec, dev_str, False, True), oracle_run(spec, dev_str))
    print(f"[engine] first_step = {first_step(spec)}: the guidance column read at the executed step moves the fp32 oracle by "
          f"rel_l2={apart:.3e} (needs >= {20 * TOL_L2:.1e})")
    assert apart >= 20 * TOL_L2, f"the two indexings are {apart:.3e} apart only: {spec}"


def assert_features_matter(spec, dev_str="cpu", guidance_vs=None, skip=()):
    """the thresholds of the features' own tests: 20 * TOL_L2 for FreeU and guidance_rescale (tests/test_gpu_freeu.py),
    lora_cases.MATTERS for a LoRA.  ``guidance_vs``: the generation is there because ``spec`` and the same spec at that
    guidance_scale differ (the single pass against the CFG path): the two fp32 oracle runs are 20 * TOL_L2 apart, the
    threshold of test_gpu_lcm.test_tiny_lcm_with_guidance_takes_the_cfg_path"""
    from conftest import TOL_L2, rel_l2
    from lora_cases import MATTERS
    need = {"freeu": 20 * TOL_L2, "rescale": 20 * TOL_L2, "loras": MATTERS, "guidance": 20 * TOL_L2, "sag": 20 * TOL_L2}
    moves = {k: v for k, v in features_moved(spec, dev_str).items() if k not in skip}
    if "pag" in moves:          # tests/test_gpu_pag.py: ten times the tolerance the trajectory is held to
        ref, arm = oracle_pair(spec.but(callback=False), dev_str)
        need["pag"] = 10 * max(TOL_L2, 1.5 * rel_l2(arm, ref))
    if guidance_vs is not None:
        assert guidance_vs != spec.guidance
        spec = spec.but(callback=False)
        moves["guidance"] = rel_l2(oracle_run(spec, dev_str), oracle_run(spec.but(guidance=guidance_vs), dev_str))
    for k, moved in moves.items():
        what = f"guidance_scale {spec.guidance} against {guidance_vs}" if k == "guidance" else k
        print(f"[engine] {what} moves the fp32 oracle of this spec by rel_l2={moved:.3e} (needs >= {need[k]:.1e})")
        assert moved >= need[k], f"{what} moves the fp32 oracle by {moved:.3e} < {need[k]:.1e}: the comparison would be vacuous for {spec}"



# --------------------------------------------------------------------------- the SAG threshold trap (tests/test_gpu_sag.py)
SAG_ARM_FACTOR = 4.0        # condition (c) against the GPU's stock fp16 arm
SAG_SEARCH_FACTOR = 10.0    # ... against the CPU stand-in (``dev_str`` "cpu"), whose deviation is 2 - 4 times smaller: the seed search's


@functools.lru_cache(maxsize=None)
def sag_figures(spec, dev_str):
    """conditions (a) - (c) of tests/test_gpu_sag.py's docstring on the reference alone -> dict(moved, fractions, margin,
    dev_arm): how far SAG moves the fp32 oracle, the mask cells set per evaluation, min |mass - 1| over the trajectory, the
    largest deviation of the fp16 arm's masses from the fp32 oracle's (on "cpu": of a CPU fp16 copy, the stand-in)"""
    import numpy as np
    from conftest import rel_l2
    spec = spec.but(callback=False)
    masses, masks, _ = guidance_trace(spec, dev_str)
    arm_masses, _, _ = guidance_trace(spec, dev_str, True)
    assert len(masses) == len(arm_masses) == executed_steps(spec)
    return dict(moved=rel_l2(oracle_run(spec, dev_str), oracle_run(spec.but(sag=0.0), dev_str)),
                fractions=[float(m.mean()) for m in masks], margin=min(float(np.abs(m - 1.0).min()) for m in masses),
                dev_arm=max(float(np.abs(a - m).max()) for a, m in zip(arm_masses, masses)))


def assert_sag_reference(spec, dev_str, factor=None):
    from conftest import TOL_L2
    factor = factor or (SAG_ARM_FACTOR if torch.device(dev_str).type == "cuda" else SAG_SEARCH_FACTOR)
    f = sag_figures(spec, dev_str)
    brief = ", ".join(f"{k.name}={getattr(spec, k.name)!r}" for k in fields(Spec) if getattr(spec, k.name) != getattr(Spec(), k.name))
    print(f"[sag] Spec({brief}): (a) SAG moves the fp32 oracle by rel_l2={f['moved']:.3e} (needs >= {20 * TOL_L2:.1e}); (b) mask cells set "
          f"per evaluation {[round(x, 3) for x in f['fractions']]} (needs 1/8 .. 7/8); (c) min |mass - 1| = {f['margin']:.3e}, largest "
          f"mass deviation of the fp16 arm {f['dev_arm']:.3e} (needs a factor {factor}, has {f['margin'] / max(f['dev_arm'], 1e-30):.1f})")
    assert f["moved"] >= 20 * TOL_L2, f"SAG moves the reference by {f['moved']:.3e} only: {spec}"
    assert all(1 / 8 <= x <= 7 / 8 for x in f["fractions"]), f"mask fractions {f['fractions']}: {spec}"
    assert f["margin"] >= factor * f["dev_arm"], f"min |mass - 1| = {f['margin']:.3e} < {factor} x {f['dev_arm']:.3e}: {spec}"
    return f


def check_masses(eng, spec, dev_str, dev_arm, what):
    """``check_last_masses`` against the reference trajectory of ``spec``"""
    check_last_masses(eng, guidance_trace(spec, dev_str)[0], dev_arm, what)


def check_last_masses(eng, masses, dev_arm, what):
    """the engine's masses of the last evaluation against the reference's (``masses``: per evaluation): the mask cells agree
    exactly, and no mass is further from the reference's than 1.5 x ``dev_arm``, the largest deviation of the fp16 arm anywhere
    on the trajectory -- the figure condition (c) of tests/test_gpu_sag.py is stated in, with check_vs_fp16_arm's slack; with (c)
    it leaves a factor 4 / 1.5 before a cell could flip.  (The arm's error on the 4 - 16 cells of ONE evaluation is too noisy an
    estimate to bound against: it moved by a third between runs.)"""
    got, want = eng.sag_mass.cpu().double(), torch.from_numpy(masses[-1])
    assert tuple(got.shape) == tuple(want.shape), f"{what}: sag_mass {tuple(got.shape)}, reference {tuple(want.shape)}"
    assert torch.equal(got > 1.0, want > 1.0), f"{what}: {int(((got > 1.0) != (want > 1.0)).sum())} mask cells differ"
    off = float((got - want).abs().max())
    print(f"[parity] {what}, masses of the last evaluation: largest deviation {off:.3e} | fp16 arm over the trajectory {dev_arm:.3e} "
          f"-> tol {1.5 * dev_arm:.3e}")
    assert torch.isfinite(got).all() and off <= 1.5 * dev_arm, f"{what}: a mass deviates by {off:.3e} > 1.5 x {dev_arm:.3e}"


def check_first_masses(got, spec, dev_str, what, trajectory_arm=False):
    """the engine's masses of evaluation 0 against the reference's, as tests/test_gpu_sag.py's two-sample cases are held: no
    trajectory lies before them, so no flipped cell can: every mass within 1.5 x the fp16 arm's largest deviation at that
    evaluation, every mask cell further than 4 x that deviation from the threshold equal, and at least half the cells are such.
    ``trajectory_arm``: where condition (c) holds the arm's trajectory is the reference's, and its largest deviation over ALL
    evaluations is the steadier figure (``check_last_masses``).  It is the looser one too: the arm drifts along a trajectory, so
    its deviation at evaluation 0 alone is up to five times smaller (1.0e-3 against 5.0e-3 on the CPU for the DPM-Solver++
    v-prediction row), and ``check_last_masses`` then applies nearly the same bound again.  What this check adds on such a
    generation is the evaluation it looks at, not a tighter figure."""
    import numpy as np
    want = torch.from_numpy(guidance_trace(spec, dev_str)[0][0])
    ref, arm = guidance_trace(spec, dev_str)[0], guidance_trace(spec, dev_str, True)[0]
    dev_arm = max(float(np.abs(a - m).max()) for a, m in (zip(arm, ref) if trajectory_arm else [(arm[0], ref[0])]))
    got = got.cpu().double()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: sag_mass {tuple(got.shape)}, reference {tuple(want.shape)}"
    off = float((got - want).abs().max())
    clear = (want - 1.0).abs() > 4.0 * dev_arm
    print(f"[parity] {what}, masses of the first evaluation: largest deviation {off:.3e} | fp16 arm {dev_arm:.3e} -> tol {1.5 * dev_arm:.3e}; "
          f"{int(clear.sum())} of {want.numel()} cells are further than 4 x that from 1")
    assert torch.isfinite(got).all() and off <= 1.5 * dev_arm, f"{what}: a mass of the first evaluation deviates by {off:.3e} > 1.5 x {dev_arm:.3e}"
    assert int(clear.sum()) >= want.numel() // 2 and torch.equal((got > 1.0)[clear], (want > 1.0)[clear]), f"{what}: mask cells differ"


# --------------------------------------------------------------------------- a scenario: generations on one live pipeline
@dataclass
class Gen:
    what: str                       # the one thing that differs from the generation before
    spec: Spec
    oracle: bool = False            # follows a change of net or UNet (the first and last generation are checked anyway)
    same_graphs: bool = False       # a transition the engine promises not to re-capture for
    pipe: Any = None                # scenarios over several pipelines: the one this generation runs on
    before: Optional[Callable[[], None]] = None     # runs first (e.g. loads an adapter)
    guidance_vs: Optional[float] = None             # the point is that this guidance_scale would differ (assert_features_matter)
    after: Optional[Callable[[Any], None]] = None   # runs last, on the engine (e.g. looks at its static buffers)
    extra: Optional[dict] = None    # further keywords of the call (``call_pipeline``); the fresh eager run is made without them
    # a SAG generation whose reference has a mass too near 1 for a trajectory to be compared: held to the fresh eager bits, to
    # the reference's masses of its FIRST evaluation (``check_first_masses``, as every SAG generation is) and to the features'
    # thresholds on the fp32 oracle, none of which needs a margin
    bits_only: bool = False
    # strength < 1 under a guidance: the point is that the guidance's per-step column is read at the schedule entry -- the
    # reference with it read at the executed step (``oracle_run(misindexed=True)``) is 20 * TOL_L2 away; asserted in place of
    # "the guidance moves the oracle", which a PAG scale that is zero in every executed step does not
    misindexed: bool = False


def run_scenario(dev, scenario, gens, pipe=None, net_objects=None):
    """-> the latents of every generation.  A SAG generation is called with a host callback that clones ``eng.sag_mass`` after
    step 0 (``check_first_masses``); the fresh eager run it is compared with has none.  The engine calls a callback between two
    launches and hands it the latents only, so the bits cannot differ -- but no scenario here replays a SAG graph WITHOUT a
    host callback between the replays: tests/test_gpu_sag.py's trajectories and its graph-equals-eager test do that."""
    assert all(executed_steps(g.spec) >= 3 for g in gens)
    outs, held, multis, last = [], [], {}, {}
    for n, g in enumerate(gens):
        p, spec = g.pipe or pipe, g.spec
        eng = p._engine
        if g.before is not None:
            g.before()
        apply_features(p, spec)         # (nothing is called where ``before`` or the generation before left the spec's state)
        if id(p) not in last or scheduler_key(last[id(p)]) != scheduler_key(spec):
            p.scheduler = product_scheduler(spec)
        if spec.nets and (id(p) not in last or (last[id(p)].nets, last[id(p)].multi) != (spec.nets, spec.multi)):
            key = (spec.nets, spec.multi)
            if key not in multis:
                multis[key] = controlnet_of(spec, net_objects)
            p.controlnet = multis[key]
            held.append(p.controlnet)
        last[id(p)] = spec
        before = len(eng.captures)
        first_masses = []       # SAG: the masses of evaluation 0, which depend on the inputs alone
        watch = (lambda i: first_masses.append(eng.sag_mass.clone()) if i == 0 else None) if spec.sag > 0.0 else None
        got, steps = call_pipeline(p, spec, dev, g.extra, watch)
        got = got.clone()
        print(f"[engine] {scenario}: generation {n} ({g.what}): captures {before} -> {len(eng.captures)}"
              f"{' (promised: none)' if g.same_graphs else ''}; graphs now {sorted(eng._graphs)}")
        rows = unet_rows(spec)
        assert eng.step_path == expected_step_path(spec), f"{scenario}, generation {n} ({g.what}): step launch {eng.step_path}"
        assert tuple(eng._static["kvrow"].shape) == (rows,), f"{scenario}, generation {n} ({g.what}): the UNet ran {tuple(eng._static['kvrow'].shape)} rows"
        want, want_steps = fresh_eager(spec, str(dev))
        assert torch.isfinite(got.float()).all(), f"{scenario}, generation {n} ({g.what}): not finite"
        assert torch.equal(got, want), (f"{scenario}, generation {n} ({g.what}): differs from the fresh eager run, max |diff| = "
                                        f"{(got.float() - want.float()).abs().max():.3e}")
        if spec.callback:
            assert len(steps) == len(want_steps) == executed_steps(spec)
            for i, (a, b) in enumerate(zip(steps, want_steps)):
                assert torch.equal(a, b), f"{scenario}, generation {n} ({g.what}): step {i} differs from the fresh eager run"
        if spec.sag > 0.0:
            check_first_masses(first_masses[0], spec, str(dev), f"{scenario}, generation {n} ({g.what})", not g.bits_only)
        if (g.oracle or n in (0, len(gens) - 1)) and g.bits_only:
            assert_features_matter(spec, str(dev), g.guidance_vs)
        if (g.oracle or n in (0, len(gens) - 1)) and not g.bits_only:
            if spec.sag > 0.0:
                figures = assert_sag_reference(spec, str(dev))
            if g.misindexed:
                assert_misindexed_differs(spec, str(dev))
            assert_features_matter(spec, str(dev), g.guidance_vs, skip=("pag", "sag") if g.misindexed else ())
            check_vs_fp16_arm(got, *oracle_pair(spec.but(callback=False), str(dev)), f"{scenario}, generation {n} ({g.what})")
            if spec.sag > 0.0:
                check_masses(eng, spec, str(dev), figures["dev_arm"], f"{scenario}, generation {n} ({g.what})")
        if spec.sag > 0.0:
            hm, wm = mid_size(spec)
            assert eng.sag_mass is not None and tuple(eng.sag_mass.shape) == (spec.B, hm * wm), f"{scenario}, generation {n}: sag_mass"
            assert torch.isfinite(eng.sag_mass).all()
        if g.same_graphs:
            assert len(eng.captures) == before, f"{scenario}, generation {n} ({g.what}): re-captured {eng.captures[before:]}"
        if g.after is not None:
            g.after(eng)
        outs.append(got)
    for p in {id(g.pipe or pipe): g.pipe or pipe for g in gens}.values():
        assert p._engine.captures, f"{scenario}: nothing was ever captured, so nothing was replayed"
    return outs
