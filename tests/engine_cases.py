"""Test-only harness for the denoise engine's state machine: the tiny models (SD1.5 UNet, two ControlNets, SDXL UNet), their
fp32 oracles and fp16 arms built once; a generation as a small frozen ``Spec``; the inputs, the pipeline call, a fresh eager
run and the oracle pair of a spec, each memoised per spec and left unchanged.  tests/test_gpu_engine_reuse.py runs lists
of specs on one live pipeline; tests/test_gpu_multicontrolnet.py takes its models and loop inputs from here."""
import functools
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch

from conftest import dev_half, half_arm
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


def new_unet(dev_str, name="tiny", adapter=0, keep_base=False):
    from consistentid_amd.unet import HipUNet
    cfg, sd, ad, _, _ = unet_models(dev_str, name, adapter)
    return HipUNet(cfg, sd, ad, device=torch.device(dev_str), keep_base=keep_base)


def new_net(dev_str, label):
    return models(dev_str)["new_cn"](list(NET_SEEDS).index(label))


# --------------------------------------------------------------------------- a generation
@dataclass(frozen=True)
class Spec:
    pipe: str = "txt2img"                       # "txt2img" | "inpaint" | "controlnet" (SD1.5 tiny) | "sdxl" (SDXL tiny)
    scheduler: str = "ddim"                     # "ddim" | "euler" | "dpm" | "pndm"
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

    def but(self, **kw):
        return replace(self, **kw)

    @property
    def name(self):
        return "tinyxl" if self.pipe == "sdxl" else "tiny"


def pipeline_class(spec):
    from consistentid_amd import pipeline
    return {"txt2img": pipeline.ConsistentIDStableDiffusionPipeline, "sdxl": pipeline.ConsistentIDStableDiffusionXLPipeline,
            "inpaint": pipeline.StableDiffusionInpaintConsistentIDPipeline,
            "controlnet": pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline}[spec.pipe]


def product_scheduler(spec):
    from consistentid_amd import scheduler
    return {"ddim": scheduler.DDIMScheduler, "euler": scheduler.EulerDiscreteScheduler,
            "dpm": scheduler.DPMSolverMultistepScheduler, "pndm": scheduler.PNDMScheduler}[spec.scheduler]()


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


def call_pipeline(pipe, spec, dev):
    """one generation of ``spec`` on ``pipe`` (whose controlnet attribute is already the spec's) -> (latents, [per-step clones])"""
    inp = inputs(spec, str(dev))
    d = lambda t: t.to(dev)
    steps = []
    kw = dict(prompt_embeds=d(torch.cat([inp["null"], inp["augmented"], inp["text"]])), latents=d(inp["latents"]),
              num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge, output_type="latent")
    if spec.callback:
        kw["callback"] = lambda i, t, lat: steps.append(lat.clone())
    if spec.eta > 0.0:
        kw.update(eta=spec.eta, variance_noise=d(inp["variance_noise"]))
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
    out = pipe(**kw).images
    torch.cuda.synchronize()
    return out, steps


def controlnet_of(spec, net_objects):
    """the pipeline's ``controlnet`` for ``spec`` out of {label: HipControlNet}"""
    from consistentid_amd.controlnet import HipMultiControlNet
    if not spec.nets:
        return None
    return HipMultiControlNet([net_objects[k] for k in spec.nets]) if spec.multi else net_objects[spec.nets[0]]


@functools.lru_cache(maxsize=None)
def fresh_eager(spec, dev_str):
    """``spec`` on objects nothing else has touched: a new HipUNet, new HipControlNets from the same state dicts, a new
    pipeline with use_graph=False -> (latents, [per-step clones])"""
    dev = torch.device(dev_str)
    kw = {}
    if spec.pipe == "controlnet":
        kw["controlnet"] = controlnet_of(spec, {k: new_net(dev_str, k) for k in spec.nets})
    pipe = pipeline_class(spec)(new_unet(dev_str, spec.name, spec.adapter), scheduler=product_scheduler(spec), use_graph=False, **kw)
    out, steps = call_pipeline(pipe, spec, dev)
    assert not pipe._engine.captures
    return out.clone(), steps


@functools.lru_cache(maxsize=None)
def oracle_pair(spec, dev_str):
    """(fp32 oracle latents, fp16-arm latents) of ``spec`` from oracle.loop.denoise"""
    from multistep_ref import DDIMEtaRef, DPMSolverPP2MRef, PNDMRef
    from oracle import ddim, loop
    dev = torch.device(dev_str)
    M = models(dev_str)
    _, _, _, o_unet, a_unet = unet_models(dev_str, spec.name, spec.adapter)
    inp = inputs(spec, dev_str)
    noises = list(inp["variance_noise"].float())

    def scheduler():
        if spec.eta > 0.0:
            assert spec.scheduler == "ddim"
            return DDIMEtaRef(spec.eta, noises)
        sch = {"ddim": ddim.DDIMScheduler, "euler": ddim.EulerDiscreteScheduler, "dpm": DPMSolverPP2MRef, "pndm": PNDMRef}[spec.scheduler]()
        sch.set_timesteps(spec.steps)       # the pipelines set the timesteps before scaling the initial noise (ref :510, :517)
        return sch

    out = []
    nets_of = lambda pool: [pool[list(NET_SEEDS).index(k)] for k in spec.nets]
    for unet, nets, f in ((o_unet, nets_of(M["o_cns"]), lambda t: t.float()), (a_unet, nets_of(M["a_cns"]), lambda t: dev_half(t, dev))):
        sch = scheduler()
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
        out.append(loop.denoise(unet, sch, f(inp["latents"]) * float(sch.init_noise_sigma), f(inp["null"]), f(inp["augmented"]),
                                f(inp["text"]), **kw))
        assert wrap is None or wrap.calls == executed_steps(spec)
    return tuple(out)
