"""Test-only helpers for community LoRA files (consistentid_amd/lora.py): a synthetic LoRA with one delta for every
LoRA-able module of a model, writers for every key spelling the loader reads, state dicts with the deltas merged in
float64 for the oracles, and the condition that keeps the parity tests from being vacuous (``assert_matters``)."""
import functools
from collections import OrderedDict

import torch

from conftest import TOL_L2, rel_l2

# the fp32 oracle with a LoRA merged must differ from the base oracle by at least this (relative L2) on the test inputs
MATTERS = 20 * TOL_L2

# sigma of ``up ~ N(0, sigma^2)``, chosen once on the CPU (fp32 oracles on the tests' own inputs) so that ``assert_matters``
# holds for every case of tests/test_gpu_lora.py -- all modules at once (about 0.2 at weight 0.7) and each module kind alone
# (0.03 for attn1.to_k, the weakest) -- while the deltas stay a fraction of the base weights (std ~0.05 at these widths)
SIGMA = 0.01


def synthetic_lora(shapes, seed, sigma, alphas=True, kinds=None):
    """``{path: (down, up, alpha)}`` over ``shapes`` = {module path: (out, in)} (only paths ending in one of ``kinds``, if
    given): ranks 4 and 16 alternate, alpha is 2 for rank 4 and 16 for rank 16 and absent on every third module (never with
    ``alphas=False``: the diffusers spellings carry none), down ~ N(0, 1 / r), up ~ N(0, sigma^2), rounded to fp16"""
    g = torch.Generator().manual_seed(seed)
    out = OrderedDict()
    for path, (o, n) in shapes.items():
        if kinds is not None and not path.endswith(tuple("." + k for k in kinds)):
            continue
        i = len(out)
        r = 4 if i % 2 == 0 else 16
        alpha = None if (not alphas or i % 3 == 2) else (2.0 if r == 4 else 16.0)
        down = (torch.randn(r, n, generator=g) * r ** -0.5).half()
        up = (torch.randn(o, r, generator=g) * sigma).half()
        out[path] = (down, up, alpha)
    ranks = {d.shape[0] for d, _, _ in out.values()}
    assert len(out) < 2 or ranks == {4, 16}
    return out


def to_kohya(modules, prefix="lora_unet_", name_of=None, conv=False):
    """kohya spelling; ``name_of``: module path -> name (default: dots to underscores; lora.sgm_path for SDXL files);
    ``conv``: proj_in / proj_out tensors shaped like 1x1 convolutions (SD1.5)"""
    flat = {}
    for path, (down, up, alpha) in modules.items():
        name = prefix + (name_of(path) if name_of else path).replace(".", "_")
        if conv and path.endswith((".proj_in", ".proj_out")):
            down, up = down[:, :, None, None], up[:, :, None, None]
        flat[name + ".lora_down.weight"], flat[name + ".lora_up.weight"] = down, up
        if alpha is not None:
            flat[name + ".alpha"] = torch.tensor(alpha)
    return flat


def to_diffusers(modules, prefix="unet.", style="peft"):
    """diffusers spellings: "peft" (lora_A / lora_B), "lora" (.lora.down / .lora.up), "layer" (.lora_linear_layer.down / .up)"""
    a, b = {"peft": (".lora_A.weight", ".lora_B.weight"), "lora": (".lora.down.weight", ".lora.up.weight"),
            "layer": (".lora_linear_layer.down.weight", ".lora_linear_layer.up.weight")}[style]
    flat = {}
    for path, (down, up, alpha) in modules.items():
        assert alpha is None, "the diffusers spellings carry no alpha"
        flat[prefix + path + a], flat[prefix + path + b] = down, up
    return flat


def delta64(down, up, alpha):
    d = up.double() @ down.double()
    return d if alpha is None else d * (alpha / down.shape[0])


def merged_state_dict(sd, entries, strip=""):
    """``sd`` in fp32 with sum_a weight_a * delta_a of ``entries`` = [(modules, weight), ...] added (float64 arithmetic);
    ``strip``: a prefix of the module paths that the state dict's keys do not have"""
    out = {k: v.detach().clone().float() for k, v in sd.items()}
    for modules, weight in entries:
        for path, (down, up, alpha) in modules.items():
            k = path[len(strip):] + ".weight"
            out[k] = (out[k].double() + weight * delta64(down, up, alpha).reshape(out[k].shape)).float()
    return out


def assert_matters(ref_lora, ref_base, what):
    """the condition under which a parity test against ``ref_lora`` says something: the LoRA moved the oracle's output"""
    moved = rel_l2(ref_lora, ref_base)
    print(f"[lora] {what}: the merged oracle differs from the base oracle by rel_l2={moved:.3e} (needs >= {MATTERS:.1e})")
    assert moved >= MATTERS, f"{what}: the LoRA moves the oracle by {moved:.3e} < {MATTERS:.1e}: the parity test would be vacuous"


# --------------------------------------------------------------------------- UNet cases
@functools.lru_cache(maxsize=None)
def unet_lora(name, seed=11, kind=None, alphas=True):
    """the synthetic LoRA of model ``name`` ("tiny" / "tinyxl"): all modules, or one module kind; built once per argument set
    and left unchanged"""
    from consistentid_amd import lora
    from oracle_utils import product_cfg
    return synthetic_lora(lora.unet_modules(product_cfg(name)), seed, SIGMA, alphas=alphas, kinds=None if kind is None else (kind,))


def forward_inputs(name, B=2):
    """one CFG-shaped UNet call (2B rows): (latents, timestep, encoder_hidden_states, added_cond_kwargs or {}) on the CPU"""
    from consistentid_amd import synth
    from oracle_utils import product_cfg
    cfg = product_cfg(name)
    side = cfg.sample_size * 8
    inp = synth.random_inputs(cfg, B, side, side)
    kw = {}
    if name == "tinyxl":
        kw = dict(added_cond_kwargs={"text_embeds": torch.cat([inp["pooled_null"], inp["pooled_text"]]), "time_ids": inp["time_ids"]})
    return torch.cat([inp["latents"]] * 2), 501, torch.cat([inp["null"], inp["text"]]), kw


def oracle_forward(unet, name, f):
    """``unet`` (an oracle in fp32, or its fp16 arm) on ``forward_inputs``; ``f`` puts a tensor where the model lives"""
    lat, t, ehs, kw = forward_inputs(name)
    kw = {k: {a: f(b) for a, b in v.items()} for k, v in kw.items()}
    with torch.no_grad():
        return unet(f(lat), t, f(ehs), **kw).sample


def hip_forward(hip, name, dev):
    lat, t, ehs, kw = forward_inputs(name)
    kw = {k: {a: b.to(dev) for a, b in v.items()} for k, v in kw.items()}
    out = hip(lat.to(dev), t, encoder_hidden_states=ehs.to(dev), cross_attention_kwargs={}, **kw).sample
    torch.cuda.synchronize()
    return out


def oracle_loop(unet, spec, f, dev_str):
    """``oracle.loop.denoise`` of an engine_cases.Spec ("txt2img" / "sdxl", DDIM) on ``unet``"""
    from engine_cases import inputs
    from oracle import ddim, loop
    inp = inputs(spec, dev_str)
    sch = ddim.DDIMScheduler()
    sch.set_timesteps(spec.steps)
    kw = dict(num_inference_steps=spec.steps, guidance_scale=spec.guidance, start_merge_step=spec.merge)
    if spec.pipe == "sdxl":
        kw.update(add_text_embeds_null=f(inp["pooled_null"]), add_text_embeds_text=f(inp["pooled_text"]),
                  add_text_embeds_aug=f(inp["pooled_augmented"]), add_time_ids=f(inp["time_ids"]))
    return loop.denoise(unet, sch, f(inp["latents"]) * float(sch.init_noise_sigma), f(inp["null"]), f(inp["augmented"]),
                        f(inp["text"]), **kw)
