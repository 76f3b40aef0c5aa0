"""Community LoRA files on the GPU: ``load_lora_weights`` / ``set_adapters`` / ``fuse_lora`` / ``unload_lora_weights`` of the
pipelines merge into the packed weights of the UNet and the text towers in place.  What the kernels then compute is held to
the fp32 oracle built from a state dict with the same deltas merged (float64) and to that oracle's fp16 arm
(conftest.check_vs_fp16_arm, defaults); every restore is held to the bits.  Tiny models, 3-step generations."""
import functools

import pytest
import torch

import lora_cases as L
from conftest import check_vs_fp16_arm, half_arm
from engine_cases import Spec, call_pipeline, fresh_eager, unet_models
from oracle_utils import build_oracle, product_cfg

pytestmark = pytest.mark.gpu

KINDS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
         "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out")
SPECS = {"tiny": Spec(steps=3, merge=1, guidance=5.0), "tinyxl": Spec(pipe="sdxl", steps=3, merge=1, guidance=7.5)}


# --------------------------------------------------------------------------- shared, built once, left unchanged
def _modules(name, key):
    """``key`` = ((seed, kind or None, alphas, weight), ...) -> the entries [(modules, weight), ...]"""
    return [(L.unet_lora(name, seed=seed, kind=kind, alphas=alphas), w) for seed, kind, alphas, w in key]


@functools.lru_cache(maxsize=None)
def _oracles(dev_str, name, key):
    """(fp32 oracle, fp16 arm) of model ``name`` with the LoRA entries of ``key`` merged (``key`` = (): the base)"""
    cfg, sd, ad, base, arm = unet_models(dev_str, name)
    if not key:
        return base, arm
    o = build_oracle(name, L.merged_state_dict(sd, _modules(name, key)), ad, rank=8)
    return o, half_arm(o, torch.device(dev_str))


@functools.lru_cache(maxsize=None)
def _forward_refs(dev_str, name, key):
    """(fp32 oracle output, fp16 arm output) of the one forward of lora_cases.forward_inputs"""
    o, arm = _oracles(dev_str, name, key)
    dev = torch.device(dev_str)
    return L.oracle_forward(o, name, lambda t: t.float()), L.oracle_forward(arm, name, lambda t: t.to(dev).half() if t.is_floating_point() else t.to(dev))


def _refs_that_matter(dev, name, key, what):
    ref, arm = _forward_refs(str(dev), name, key)
    L.assert_matters(ref, _forward_refs(str(dev), name, ())[0], what)
    return ref, arm


def _pipe(dev, name="tiny", adapter=True, keep_base=True, use_graph=False, **kw):
    from consistentid_amd import pipeline
    from consistentid_amd.unet import HipUNet
    cfg, sd, ad, _, _ = unet_models(str(dev), name)
    unet = HipUNet(cfg, sd, ad if adapter else None, device=dev, keep_base=keep_base)
    cls = pipeline.ConsistentIDStableDiffusionXLPipeline if name == "tinyxl" else pipeline.ConsistentIDStableDiffusionPipeline
    return cls(unet, use_graph=use_graph, **kw)


def _file(name, modules):
    """the LoRA as a kohya file of its family: SD1.5 with 1x1-convolution shaped proj_in / proj_out, SDXL with SGM names"""
    from consistentid_amd import lora
    if name == "tinyxl":
        cfg = product_cfg(name)
        return L.to_kohya(modules, name_of=lambda p: lora.sgm_path(cfg, p))
    return L.to_kohya(modules, conv=True)


def _bits(unet):
    return {k: v.view(torch.int16).clone() for k, v in unet.W.items()}


def _ptrs(unet):
    return {k: v.data_ptr() for k, v in unet.W.items()}


def _same_bits(unet, snap, what):
    torch.cuda.synchronize()
    bad = [k for k, v in unet.W.items() if not torch.equal(v.view(torch.int16), snap[k])]
    assert not bad, f"{what}: {len(bad)} packed tensors differ, e.g. {bad[:3]}"


# --------------------------------------------------------------------------- 1. UNet parity
@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_unet_parity(dev, name):
    """tiny at 32 x 32 latents, tinyxl at 16 x 16, B = 2: one forward and a 3-step generation with the LoRA at weight 0.7"""
    key = ((11, None, True, 0.7),)
    pipe = _pipe(dev, name)
    pipe.load_lora_weights(_file(name, L.unet_lora(name)), adapter_name="A")
    pipe.set_adapters("A", 0.7)
    ref, arm = _refs_that_matter(dev, name, key, f"{name} forward, LoRA x 0.7")
    check_vs_fp16_arm(L.hip_forward(pipe.unet, name, dev), ref, arm, f"{name} UNet forward with LoRA x 0.7")
    spec = SPECS[name]
    o, a = _oracles(str(dev), name, key)
    want = L.oracle_loop(o, spec, lambda t: t.float(), str(dev))
    L.assert_matters(want, L.oracle_loop(_oracles(str(dev), name, ())[0], spec, lambda t: t.float(), str(dev)), f"{name} 3-step loop")
    want16 = L.oracle_loop(a, spec, lambda t: t.to(dev).half() if t.is_floating_point() else t.to(dev), str(dev))
    got, _ = call_pipeline(pipe, spec, dev)
    check_vs_fp16_arm(got, want, want16, f"{name} 3-step generation with LoRA x 0.7")


# --------------------------------------------------------------------------- 2. every module counts
@functools.lru_cache(maxsize=None)
def _base_engine_forward(dev_str):
    dev = torch.device(dev_str)
    return L.hip_forward(_pipe(dev, "tiny").unet, "tiny", dev).clone()


@pytest.mark.parametrize("kind", KINDS)
def test_every_module_kind_counts(dev, kind):
    """a LoRA that holds one module kind only: a derived tensor that was not rebuilt (ffpo, the LayerNorm-folded copies) would
    leave the engine at the base's output or off its oracle"""
    pipe = _pipe(dev, "tiny")
    modules = L.unet_lora("tiny", kind=kind)
    assert modules and all(p.endswith("." + kind) for p in modules)
    pipe.load_lora_weights(_file("tiny", modules))
    ref, arm = _refs_that_matter(dev, "tiny", ((11, kind, True, 1.0),), f"tiny forward, {kind} only")
    got = L.hip_forward(pipe.unet, "tiny", dev)
    check_vs_fp16_arm(got, ref, arm, f"tiny UNet forward with a LoRA on {kind} only")
    assert not torch.equal(got, _base_engine_forward(str(dev))), f"{kind}: the engine's output is the base engine's"


# --------------------------------------------------------------------------- 3. exact restores
def test_exact_restores(dev):
    pipe = _pipe(dev, "tiny")
    unet = pipe.unet
    snap, ptrs = _bits(unet), _ptrs(unet)
    flat = _file("tiny", L.unet_lora("tiny"))
    pipe.load_lora_weights(flat, adapter_name="A")
    assert _ptrs(unet) == ptrs, "load_lora_weights moved a packed tensor"
    first = _bits(unet)
    changed = sorted({k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1] for k in snap if not torch.equal(first[k], snap[k])})
    print(f"[lora] packed tensors a full LoRA changes: {changed}")
    # every tensor derived from a LoRA-able weight (the tiny widths have no wq_f / wq_p / wo_p / qs / qb), and nothing else: no
    # bias, no norm, not kv_ip
    assert changed == sorted(["qkv.w", "qkv.wl", "qkv.lns", "qkv.lnb", "out.w", "attn2.wq", "attn2.wql", "attn2.wq_lns",
                              "attn2.wq_lnb", "attn2.wo", "kv_txt.w", "ff1.w", "ff1.wl", "ff1.lns", "ff1.lnb", "ff2.w", "proj_in.w",
                              "proj_out.w", "ffpo.w", "ffpo.b"])
    pipe.unload_lora_weights()
    _same_bits(unet, snap, "unload_lora_weights")
    pipe.load_lora_weights(flat, adapter_name="A")
    _same_bits(unet, first, "load, unload, load again")
    pipe.set_adapters("A", 0.0)
    _same_bits(unet, snap, "set_adapters(name, 0.0)")
    pipe.set_adapters("A", 0.5)
    half = _bits(unet)
    assert any(not torch.equal(half[k], first[k]) for k in half)
    pipe.set_adapters("A")
    _same_bits(unet, first, "set_adapters(name)")
    pipe.fuse_lora(0.5)
    _same_bits(unet, half, "fuse_lora(0.5) against set_adapters(name, 0.5)")
    pipe.unfuse_lora()
    _same_bits(unet, first, "fuse_lora(0.5) then unfuse_lora()")
    assert _ptrs(unet) == ptrs
    pipe.unload_lora_weights()
    _same_bits(unet, snap, "the last unload_lora_weights")


# --------------------------------------------------------------------------- 4. with the ConsistentID adapter
def test_with_the_consistentid_adapter_in_either_order(dev):
    ad = unet_models(str(dev), "tiny")[2]
    flat = _file("tiny", L.unet_lora("tiny"))
    p1, p2, p3 = (_pipe(dev, "tiny", adapter=False) for _ in range(3))
    p1.load_ConsistentID_model({"adapter_modules": ad}, lora_rank=8)
    p1.load_lora_weights(flat)
    p2.load_lora_weights(flat)
    p2.load_ConsistentID_model({"adapter_modules": ad}, lora_rank=8)
    p3.load_ConsistentID_model({"adapter_modules": ad}, lora_rank=8)
    _same_bits(p2.unet, _bits(p1.unet), "LoRA then checkpoint against checkpoint then LoRA")
    assert p1.unet.packed.ip_scale == p2.unet.packed.ip_scale == p3.unet.packed.ip_scale
    ref, arm = _refs_that_matter(dev, "tiny", ((11, None, True, 1.0),), "tiny forward, checkpoint + LoRA")
    for what, p in (("checkpoint then LoRA", p1), ("LoRA then checkpoint", p2)):
        check_vs_fp16_arm(L.hip_forward(p.unet, "tiny", dev), ref, arm, f"tiny UNet forward, {what}")
    for p in (p1, p2):
        p.unload_lora_weights()
        _same_bits(p.unet, _bits(p3.unet), "unload_lora_weights against an engine that only loaded the checkpoint")


# --------------------------------------------------------------------------- 5. two adapters
def test_two_adapters(dev):
    pipe = _pipe(dev, "tiny")
    pipe.load_lora_weights(_file("tiny", L.unet_lora("tiny", seed=11)), adapter_name="A")
    pipe.load_lora_weights(L.to_diffusers(L.unet_lora("tiny", seed=12, alphas=False)), adapter_name="B")      # (peft spelling)
    pipe.set_adapters(["A", "B"], [1.0, 0.5])
    ref, arm = _refs_that_matter(dev, "tiny", ((11, None, True, 1.0), (12, None, False, 0.5)), "tiny forward, A + 0.5 B")
    check_vs_fp16_arm(L.hip_forward(pipe.unet, "tiny", dev), ref, arm, "tiny UNet forward with A + 0.5 B")
    pipe.set_adapters("B")
    assert pipe.get_active_adapters() == ["B"] and pipe.get_list_adapters() == ["A", "B"]
    ref, arm = _refs_that_matter(dev, "tiny", ((12, None, False, 1.0),), "tiny forward, B only")
    check_vs_fp16_arm(L.hip_forward(pipe.unet, "tiny", dev), ref, arm, "tiny UNet forward with B only")


# --------------------------------------------------------------------------- 6. graphs
def test_graphs_follow_the_weights(dev):
    """generate, load a LoRA, generate, unload, generate on one use_graph=True pipeline: each result is the bits of the same call
    on a fresh eager pipeline in the same LoRA state (the captured steps read the weights where they always were)"""
    spec = SPECS["tiny"]
    flat = _file("tiny", L.unet_lora("tiny"))
    pipe = _pipe(dev, "tiny", use_graph=True)
    eng = pipe._engine
    eager = _pipe(dev, "tiny", use_graph=False)
    eager.load_lora_weights(flat)
    want_lora = call_pipeline(eager, spec, dev)[0].clone()
    assert not eager._engine.captures
    want_base = fresh_eager(spec, str(dev))[0]
    assert not torch.equal(want_lora, want_base)
    outs = []
    for what, before, want in (("base", None, want_base), ("LoRA loaded", lambda: pipe.load_lora_weights(flat), want_lora),
                               ("LoRA unloaded", pipe.unload_lora_weights, want_base)):
        if before is not None:
            before()
        n = len(eng.captures)
        got = call_pipeline(pipe, spec, dev)[0].clone()
        print(f"[engine] LoRA: generation {len(outs)} ({what}): captures {n} -> {len(eng.captures)}; graphs now {len(eng._graphs)}")
        assert torch.equal(got, want), f"{what}: differs from the fresh eager run, max |diff| = {(got.float() - want.float()).abs().max():.3e}"
        outs.append(got)
    assert torch.equal(outs[2], outs[0])
    assert eng.captures, "nothing was ever captured, so nothing was replayed"


# --------------------------------------------------------------------------- 7. text towers
def _tower(dev, shape):
    """a CLIP-L-shaped (quick_gelu, no projection) or bigG-shaped (gelu, projection) tiny tower at test_gpu_clip_text's widths:
    (config, fp32 transformers model with fp16-representable weights, its state dict without the ``text_model.`` prefix)"""
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    from test_clip_text_host import tiny_text_config
    from test_gpu_clip_text import CONFIGS
    args = dict(CONFIGS["tiny"], hidden_act="quick_gelu" if shape == "clip_l" else "gelu")
    cfg = tiny_text_config(49408, eos_token_id=2, **args)
    torch.manual_seed(5)
    ref = (CLIPTextModelWithProjection if shape == "bigg" else CLIPTextModel)(cfg).eval()
    with torch.no_grad():
        for p in ref.parameters():
            if p.ndim == 1:
                p.add_(torch.randn_like(p) * 0.05)
            p.copy_(p.half().float())
    return cfg, ref


def _tower_outputs(model, ids, projection):
    with torch.no_grad():
        o = model(ids.to(next(model.parameters()).device), output_hidden_states=True)
    return [o.last_hidden_state, o.hidden_states[-2]] + ([o.text_embeds] if projection else [])


@pytest.mark.parametrize("shape", ["clip_l", "bigg"])
def test_text_tower_lora(dev, shape):
    import copy
    from consistentid_amd import lora
    from consistentid_amd.clip_text import HipCLIPTextModel
    from test_gpu_clip_text import _ids
    projection = shape == "bigg"
    cfg, ref = _tower(dev, shape)
    hip = HipCLIPTextModel(ref.state_dict(), cfg, device=dev, keep_base=True)
    name, target, prefix = ("tinyxl", "text_encoder_2", "lora_te2_") if projection else ("tiny", "text_encoder", "lora_te_")
    pipe = _pipe(dev, name, **{target: hip})
    snap, ptrs = {k: v.view(torch.int16).clone() for k, v in hip.W.items()}, {k: v.data_ptr() for k, v in hip.W.items()}
    unet_snap = _bits(pipe.unet)
    modules = L.synthetic_lora(lora.tower_modules(cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size), 21, L.SIGMA)
    unet_part = L.unet_lora(name, kind="proj_in")
    # one file holding both lora_unet_ and tower keys changes both engines
    pipe.load_lora_weights(dict(L.to_kohya(modules, prefix=prefix), **L.to_kohya(unet_part)), adapter_name="both")
    assert any(not torch.equal(v.view(torch.int16), unet_snap[k]) for k, v in pipe.unet.W.items()), "the UNet part was not merged"
    pipe.set_adapters("both", 0.7)
    sd = ref.state_dict()
    pre = "text_model." if any(k.startswith("text_model.") for k in sd) else ""
    merged = copy.deepcopy(ref)
    merged.load_state_dict(L.merged_state_dict(sd, [(modules, 0.7)], strip="" if pre else "text_model."))
    arm = half_arm(merged, dev)
    ids = _ids(3, [7, 75, 40], 0 if projection else 49407, seed=3)
    want, want16, base = _tower_outputs(merged, ids, projection), _tower_outputs(arm, ids, projection), _tower_outputs(ref, ids, projection)
    L.assert_matters(want[0], base[0], f"{shape} tower last_hidden_state, LoRA x 0.7")
    h = hip(ids, output_hidden_states=True)
    torch.cuda.synchronize()
    got = [h.last_hidden_state, h.hidden_states[-2]] + ([h.text_embeds] if projection else [])
    for what, g, w, a in zip(("last_hidden_state", "hidden_states[-2]", "text_embeds"), got, want, want16):
        check_vs_fp16_arm(g, w, a, f"{shape} tower with LoRA x 0.7, {what}")
    assert {k: v.data_ptr() for k, v in hip.W.items()} == ptrs
    pipe.unload_lora_weights()
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.int16), snap[k]) for k, v in hip.W.items()), "unload did not restore the tower's bits"
    _same_bits(pipe.unet, unet_snap, "unload_lora_weights (UNet part)")
    # a tower built without keep_base refuses before the UNet is touched
    plain = _pipe(dev, name, **{target: HipCLIPTextModel(ref.state_dict(), cfg, device=dev)})
    with pytest.raises(RuntimeError, match="keep_base"):
        plain.load_lora_weights(dict(L.to_kohya(modules, prefix=prefix), **L.to_kohya(unet_part)))
    _same_bits(plain.unet, unet_snap, "a refused load")


# --------------------------------------------------------------------------- 8. refusals leave the engine untouched
def test_refusals_leave_the_engine_untouched(dev):
    pipe = _pipe(dev, "tiny")
    snap = _bits(pipe.unet)
    flat = _file("tiny", L.unet_lora("tiny"))
    conv = {"lora_unet_mid_block_resnets_0_conv1.lora_down.weight": torch.zeros(4, 128, 3, 3),
            "lora_unet_mid_block_resnets_0_conv1.lora_up.weight": torch.zeros(128, 4, 1, 1)}
    with pytest.raises(NotImplementedError, match="mid_block_resnets_0_conv1"):
        pipe.load_lora_weights(dict(flat, **conv))
    _same_bits(pipe.unet, snap, "a refused file")
    assert pipe.get_list_adapters() == []
    plain = _pipe(dev, "tiny", keep_base=False)
    _same_bits(plain.unet, snap, "keep_base=False against keep_base=True")
    with pytest.raises(RuntimeError, match="keep_base"):
        plain.load_lora_weights(flat)
    with pytest.raises(RuntimeError, match="keep_base"):
        plain.unet.set_lora([])
    _same_bits(plain.unet, snap, "an engine without keep_base")
    assert plain.get_list_adapters() == []


# --------------------------------------------------------------------------- 9. memory
@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_keep_base_costs_no_more_device_memory(dev, name):
    """with no LoRA loaded the device bytes of a keep_base=True engine are the packed tensors plus the fp16 attention base, as
    before this feature; what is newly retained for ff.net.0.proj, ff.net.2, proj_in and proj_out lives on the host"""
    from consistentid_amd import unet_spec
    kept, plain = _pipe(dev, name).unet.packed, _pipe(dev, name, keep_base=False).unet.packed
    shapes = unet_spec.unet_param_shapes(unet_models(str(dev), name)[0])
    attn_base = sum(2 * s[0] * s[1] for k, s in shapes.items()
                    if k.endswith(tuple(f".{a}.{w}.weight" for a in ("attn1", "attn2") for w in ("to_q", "to_k", "to_v", "to_out.0"))))
    assert attn_base > 0 and kept.nbytes() == plain.nbytes()
    assert kept.retained_device_bytes() == attn_base and plain.retained_device_bytes() == 0
    assert sum(t.numel() * t.element_size() for t in kept._base_attn.values()) == attn_base
    assert kept._base_host and not any(t.is_cuda for t in kept._base_host.values())
    for module in ("ff.net.0.proj", "ff.net.2", "proj_in", "proj_out"):
        assert any(k.endswith(f".{module}.weight") for k in kept._base_host), module
