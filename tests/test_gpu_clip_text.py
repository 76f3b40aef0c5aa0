"""HIP CLIP text towers on the GPU: HipCLIPTextModel against transformers' CLIPTextModel / CLIPTextModelWithProjection
(fp32 CPU oracle, stock-fp16 arm on this GPU), causality and determinism, cid_quick_gelu_f16 over every fp16 value, the
causal attention kernel alone against fp64, and prompt strings through the pipelines end to end."""
import json

import numpy as np
import pytest
import torch

from conftest import check_close, check_vs_fp16_arm, half_arm
from test_clip_text_host import make_tokenizer_dir, tiny_text_config
from test_gpu_ranges import _assert_within_ulp16, _finite_fp16

pytestmark = pytest.mark.gpu

CONFIGS = {
    "tiny": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, hidden_act="quick_gelu",
                 projection_dim=64),
    "clip_l": dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   hidden_act="quick_gelu", projection_dim=768),
    "bigg": dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, hidden_act="gelu",
                 projection_dim=1280),
}


def _pair(dev, name, projection, eos=2, vocab=49408, seed=5):
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    from consistentid_amd.clip_text import HipCLIPTextModel
    cfg = tiny_text_config(vocab, eos_token_id=eos, **CONFIGS[name])
    torch.manual_seed(seed)
    ref = (CLIPTextModelWithProjection if projection else CLIPTextModel)(cfg).eval()
    with torch.no_grad():                       # fp16-representable weights; LayerNorm gains / biases off their init
        for n, p in ref.named_parameters():
            if p.ndim == 1:
                p.add_(torch.randn_like(p) * 0.05)
            p.copy_(p.half().float())
    return cfg, ref, HipCLIPTextModel(ref.state_dict(), cfg, device=dev)


def _ids(B, lens, pad, eos_id=49407, bos_id=49406, vocab=49406, seed=0):
    """token rows [BOS, words, EOS, pad...] of different real lengths (SD1.5 pads with EOS, OpenCLIP's tokenizer with 0)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, 77), pad, dtype=torch.long)
    for b, n in enumerate(lens[:B]):
        ids[b, 0] = bos_id
        ids[b, 1:n + 1] = torch.randint(0, vocab, (n,), generator=g)
        ids[b, n + 1] = eos_id
    return ids


def _compare(cfg, ref, arm, hip, ids, what):
    with torch.no_grad():
        o = ref(ids, output_hidden_states=True)
        a = arm(ids.to(arm.device), output_hidden_states=True)
    h = hip(ids, output_hidden_states=True)
    torch.cuda.synchronize()
    assert len(h.hidden_states) == len(o.hidden_states) == cfg.num_hidden_layers + 1
    check_vs_fp16_arm(h.last_hidden_state, o.last_hidden_state, a.last_hidden_state, f"{what} last_hidden_state")
    check_vs_fp16_arm(h.hidden_states[-2], o.hidden_states[-2], a.hidden_states[-2], f"{what} hidden_states[-2]")
    if hasattr(o, "text_embeds"):
        assert torch.equal(h[0], h.text_embeds)
        check_vs_fp16_arm(h.text_embeds, o.text_embeds, a.text_embeds, f"{what} text_embeds")
    else:
        assert torch.equal(h[0], h.last_hidden_state)
        check_vs_fp16_arm(h.pooler_output, o.pooler_output, a.pooler_output, f"{what} pooler_output")
    return h


@pytest.mark.parametrize("name,projection,eos", [("tiny", False, 2), ("tiny", True, 49407), ("clip_l", False, 2),
                                                 ("bigg", True, 2)])
def test_text_tower_matches_transformers(dev, name, projection, eos):
    """B = 1 and B = 3 with different real lengths; SD1.5-style EOS padding for CLIP-L, zero padding for bigG"""
    cfg, ref, hip = _pair(dev, name, projection, eos=eos)
    pad = 0 if name == "bigg" else 49407
    arm = half_arm(ref, dev)       # transformers' own modules in fp16 on this GPU: what the reference's pipeline runs
    for B, lens in ((1, [20]), (3, [7, 75, 40])):
        _compare(cfg, ref, arm, hip, _ids(B, lens, pad, seed=B), f"{name} B={B} eos={eos}")


def test_text_tower_is_causal_and_deterministic(dev):
    cfg, ref, hip = _pair(dev, "tiny", False)
    ids = _ids(2, [30, 60], 49407)
    p = 25
    ids2 = ids.clone()
    ids2[:, p + 1:] = torch.randint(0, 49406, (2, 76 - p))
    a = hip(ids, output_hidden_states=True)
    b = hip(ids2, output_hidden_states=True)
    c = hip(ids, output_hidden_states=True)
    torch.cuda.synchronize()
    for x, y in [(a.last_hidden_state, b.last_hidden_state)] + list(zip(a.hidden_states, b.hidden_states)):
        assert torch.equal(x[:, :p + 1], y[:, :p + 1])
    assert not torch.equal(a.last_hidden_state[:, p + 1:], b.last_hidden_state[:, p + 1:])
    assert torch.equal(a.last_hidden_state, c.last_hidden_state) and torch.equal(a.pooler_output, c.pooler_output)
    assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, c.hidden_states))


def test_quick_gelu_every_fp16_value(dev):
    from consistentid_amd import ops
    h = _finite_fp16()
    y = h.to(dev).clone()
    ops.quick_gelu_(y)
    torch.cuda.synchronize()
    x = h.double()
    _assert_within_ulp16(y, x * torch.sigmoid(1.702 * x), "quick_gelu_ over every finite fp16 value")


@pytest.mark.parametrize("smax", [None, 60.0, 600.0])
@pytest.mark.parametrize("N,n_keys", [(128, 77), (192, 150), (128, 128)])
def test_causal_attention_kernel(dev, N, n_keys, smax):
    """cid_self_attn_causal_f16 against fp64: randn scores (smax None) and wide logit ranges (|score| up to ~smax in log2
    units); real rows checked, pad query rows finite"""
    from consistentid_amd import ops
    B, heads, d = 2, 3, 64
    C = heads * d
    g = torch.Generator().manual_seed(N + n_keys)
    k = torch.randn(B, N, C, generator=g).half()
    q = (torch.randn(B, N, C, generator=g) * (0.125 if smax is None else smax / (4 * d ** 0.5))).half()
    v = torch.randn(B, N, C, generator=g).half()
    qd, kd, vd = (t.double().view(B, N, heads, d) for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", qd, kd)
    i, j = torch.arange(N)[:, None], torch.arange(N)[None, :]
    s = s.masked_fill((j > i) | (j >= n_keys), -float("inf"))
    ref = torch.einsum("bhij,bjhd->bihd", torch.softmax(s * np.log(2.0), -1), vd).reshape(B, N, C)
    t = torch.arange(N)
    pos = (t & ~15) | (8 * ((t >> 2) & 1) + 4 * ((t >> 3) & 1) + (t & 3))
    vt = torch.zeros(B, heads, d, N, dtype=torch.float16)
    vt[..., pos] = v.view(B, N, heads, d).permute(0, 2, 3, 1)
    out = torch.full((B, N, C), float("nan"), dtype=torch.float16, device=dev)
    ops.self_attn_causal(q.to(dev), k.to(dev), vt.to(dev), out, B=B, N=N, heads=heads, d=d, ldq=C, ldk=C, ldo=C,
                         n_keys=n_keys)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), "pad query rows must come out finite"
    check_close(out[:, :n_keys], ref[:, :n_keys], f"causal attn N={N} n_keys={n_keys} smax={smax}", tol_l2=2e-3,
                tol_max=8e-3)


# ----------------------------------------------------------------------------- end to end through the pipelines
def _save_tower(folder, cfg, projection, seed):
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    m = (CLIPTextModelWithProjection if projection else CLIPTextModel)(cfg).eval()
    m.save_pretrained(str(folder))
    return m


def _diffusers_encode(tok, model, texts, hidden=None):
    """diffusers 0.23's text-encoder call on the fp32 transformers oracle"""
    ids = tok(texts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    with torch.no_grad():
        o = model(ids, output_hidden_states=True)
    return o if hidden else o[0]


def test_sd15_prompt_strings_end_to_end(tmp_path, dev):
    from consistentid_amd import pipeline, synth, unet_spec
    from oracle import idstack
    from oracle_utils import idstack_weights
    from test_loader import _write_component
    cfg = unet_spec.tiny_config("sd15")
    sd = synth.random_unet_state_dict(cfg, seed=0)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=1)
    root = tmp_path / "base"
    _write_component(root / "unet", {"block_out_channels": list(cfg.block_out_channels),
                                     "down_block_types": list(cfg.down_block_types), "up_block_types": list(cfg.up_block_types),
                                     "layers_per_block": 1, "attention_head_dim": 2, "cross_attention_dim": 128,
                                     "sample_size": 32}, sd, "safetensors")
    V = make_tokenizer_dir(root / "tokenizer")
    tcfg = tiny_text_config(V, eos_token_id=2)
    ref = _save_tower(root / "text_encoder", tcfg, False, seed=7)
    pipe = pipeline.ConsistentIDStableDiffusionPipeline.from_pretrained(str(root), device=dev)
    assert pipe.text_encoder is not None and pipe.tokenizer is not None
    sd_ip = idstack_weights(idstack.ProjPlusModel(cross_attention_dim=128, id_embeddings_dim=512, clip_embeddings_dim=192), 3)
    sd_fe = idstack_weights(idstack.FacialEncoder(embedding_dim=192, output_dim=128, embed_dim=128), 4)
    pipe.load_ConsistentID_model({"adapter_modules": ad, "image_proj": sd_ip, "FacialEncoder": sd_fe}, lora_rank=8)
    tok = pipe.tokenizer
    assert tok.convert_tokens_to_ids("<|image|>") == V and tok.convert_tokens_to_ids("<|facial|>") == V + 1
    with pytest.raises(ValueError, match="outside the text encoder's embedding table"):
        pipe.encode_prompt("a <|facial|> man", do_classifier_free_guidance=False)
    # the reference's pre-loop (ref :460-507) with the HIP pieces
    text_only, clean_ids, _, fmask, _, _ = pipe.encode_prompt_with_trigger_word("a man", "The face is round.", {"Face": 1})
    text_embeds = pipe.text_encoder(clean_ids)[0]
    with torch.no_grad():
        want = ref(clean_ids)[0]
    check_close(text_embeds, want, "text_encoder(clean_input_id)[0]", tol_l2=5e-3, tol_max=2e-2)
    pos, neg = pipe.encode_prompt(text_only, dev, 1, True, None)
    check_close(pos, _diffusers_encode(tok, ref, [text_only]), "encode_prompt positive", tol_l2=5e-3, tol_max=2e-2)
    check_close(neg, _diffusers_encode(tok, ref, [""]), "encode_prompt negative", tol_l2=5e-3, tol_max=2e-2)
    legacy = pipe._encode_prompt(text_only, dev, 1, True, None)
    assert torch.equal(legacy, torch.cat([neg, pos]))
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).half()
    prompt_embeds = pipe.prepare_prompt_embeds(
        text_embeds=text_embeds, negative_embeds=neg, text_only_embeds=pos, faceid_embeds=rnd(1, 512),
        clip_embeds=rnd(1, 257, 192), uncond_clip_embeds=rnd(1, 257, 192), facial_embeds=rnd(1, 5, 257, 192),
        uncond_facial_embeds=rnd(1, 5, 257, 192), facial_token_mask=fmask,
        valid_facial_mask=torch.tensor([[True, False, False, False, False]]))
    assert prompt_embeds.shape == (3, 81, 128)
    lat = pipe(prompt_embeds=prompt_embeds, latents=torch.randn(1, 4, 32, 32, generator=g).to(dev), num_inference_steps=2,
               output_type="latent").images
    torch.cuda.synchronize()
    assert torch.isfinite(lat.float()).all()
    with pytest.raises(NotImplementedError):
        pipe(prompt="a photo of a man", input_id_images=[object()])


def test_sdxl_encode_prompt_end_to_end(tmp_path, dev):
    from consistentid_amd import pipeline, synth, unet_spec
    from test_loader import _write_component
    cfg = unet_spec.tiny_config("sdxl")
    sd = synth.random_unet_state_dict(cfg, seed=0)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=1)
    root = tmp_path / "base"
    ujson = {"block_out_channels": list(cfg.block_out_channels), "down_block_types": list(cfg.down_block_types),
             "up_block_types": list(cfg.up_block_types), "layers_per_block": cfg.layers_per_block,
             "attention_head_dim": list(cfg.num_attention_heads), "cross_attention_dim": cfg.cross_attention_dim,
             "transformer_layers_per_block": list(cfg.transformer_layers_per_block), "use_linear_projection": True,
             "addition_embed_type": "text_time", "addition_time_embed_dim": cfg.addition_time_embed_dim,
             "projection_class_embeddings_input_dim": cfg.projection_class_embeddings_input_dim, "sample_size": 32}
    _write_component(root / "unet", ujson, sd, "safetensors")
    V = make_tokenizer_dir(root / "tokenizer")
    make_tokenizer_dir(root / "tokenizer_2")
    with open(root / "model_index.json", "w") as f:
        json.dump({"force_zeros_for_empty_prompt": True}, f)
    r1 = _save_tower(root / "text_encoder", tiny_text_config(V), False, seed=11)
    r2 = _save_tower(root / "text_encoder_2", tiny_text_config(V, hidden_act="gelu"), True, seed=12)
    pipe = pipeline.ConsistentIDStableDiffusionXLPipeline.from_pretrained(str(root), device=dev)
    assert pipe.force_zeros_for_empty_prompt and pipe.text_encoder_2.with_projection
    pe, ne, pp, npool = pipe.encode_prompt("a man", num_images_per_prompt=2)
    t1, t2 = pipe.tokenizer, pipe.tokenizer_2
    o1, o2 = _diffusers_encode(t1, r1, ["a man"], True), _diffusers_encode(t2, r2, ["a man"], True)
    want = torch.cat([o1.hidden_states[-2], o2.hidden_states[-2]], -1).repeat_interleave(2, 0)
    assert pe.shape == (2, 77, 256) and pp.shape == (2, 64)
    check_close(pe, want, "SDXL prompt_embeds", tol_l2=5e-3, tol_max=2e-2)
    check_close(pp, o2[0].repeat_interleave(2, 0), "SDXL pooled", tol_l2=5e-3, tol_max=2e-2)
    assert not ne.any() and not npool.any()
    _, ne2, _, npool2 = pipe.encode_prompt("a man", negative_prompt="blurry")
    n1, n2 = _diffusers_encode(t1, r1, ["blurry"], True), _diffusers_encode(t2, r2, ["blurry"], True)
    check_close(ne2, torch.cat([n1.hidden_states[-2], n2.hidden_states[-2]], -1), "SDXL negative", tol_l2=5e-3, tol_max=2e-2)
    check_close(npool2, n2[0], "SDXL negative pooled", tol_l2=5e-3, tol_max=2e-2)
    pipe.load_ConsistentID_model({"adapter_modules": ad}, lora_rank=8)
    assert pipe.tokenizer.convert_tokens_to_ids("<|facial|>") == V + 1
    assert pipe.tokenizer_2.convert_tokens_to_ids("<|image|>") == V and "<|facial|>" not in pipe.tokenizer_2.get_vocab()
    out = pipe.encode_prompt_with_trigger_word("a man", "The face is round.", {"Face": 1})
    assert out[1].shape == out[2].shape == (1, 77) and not torch.equal(out[1], out[2])
