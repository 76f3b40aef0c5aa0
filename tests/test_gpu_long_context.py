"""Contexts beyond 96 rows through the engines: ``prompt_embeds`` of 154 / 231 text rows (+ ID tokens) on the four pipelines'
tiny models, every cross-attention layer on the long-context kernel (csrc/xattn_long.hip), the ControlNet on (T + 4) + 0
rows; one pipeline across 77 -> 231 -> 77 text rows with step graphs on; and ``encode_prompt(max_embeddings_multiples=3)``
on a tiny HipCLIPTextModel.

The generations run through engine_cases.run_scenario: bit-identical to the same spec run eagerly on fresh objects, and
within the fp16 arm of the fp32 oracle (conftest.check_vs_fp16_arm, defaults), 4 steps.

UNPINNED: the chunked / weighted encoding restates diffusers' community pipeline ``lpw_stable_diffusion`` from written rules
(tests/lpw_ref.py); the original file is not available here."""
import numpy as np
import pytest
import torch

import lpw_ref
from engine_cases import Gen, Spec, new_net, new_unet, pipeline_class, run_scenario
from fake_tokenizer import FakeTokenizer

pytestmark = pytest.mark.gpu

LONG = [Spec(text_len=154),
        Spec(pipe="sdxl", text_len=231),
        Spec(pipe="controlnet", nets=("A",), scales=(1.0,), windows=((0.0, 1.0),), text_len=154),
        Spec(pipe="inpaint", text_len=154, scheduler="dpm")]


def _pipe(dev, spec, nets=None):
    kw = {"controlnet": nets[spec.nets[0]]} if spec.nets else {}
    return pipeline_class(spec)(new_unet(str(dev), spec.name), use_graph=True, **kw)


def _long_layers(unet):
    from consistentid_amd.unet import LONG_CONTEXT
    return [v == LONG_CONTEXT for v in unet._ctx.v2.values()]


@pytest.mark.parametrize("spec", LONG, ids=lambda s: f"{s.pipe}-{s.text_len}")
def test_long_prompt_embeds(dev, spec):
    assert spec.steps == 4
    nets = {k: new_net(str(dev), k) for k in spec.nets}
    pipe = _pipe(dev, spec, nets)
    run_scenario(dev, f"{spec.pipe}, {spec.text_len} text rows", [Gen("long context", spec)], pipe, nets)
    layers = _long_layers(pipe.unet)
    assert layers and all(layers), "a cross-attention layer was not packed for the long-context kernel"
    assert pipe.unet._ctx.n_txt == spec.text_len
    paths = {pipe.unet.cross_attention_path(b, 64, 2, 64) for b in pipe.unet._ctx.v2}
    assert all("id_xattn_long core" in p for p in paths), paths
    for net in nets.values():
        layers = _long_layers(net)
        assert layers and all(layers) and (net._ctx.n_txt, net._ctx.n_ip) == (spec.text_len + 4, 0)


def test_context_length_switches_with_graphs_on(dev):
    """77 -> 231 -> 77 text rows on one live pipeline: the K/V images are resized (a new epoch) and the layout and the launch
    sequence change, so every switch re-captures; the third generation is the first one, bit for bit"""
    base = Spec()
    pipe = _pipe(dev, base)
    gens = [Gen("77 text rows", base), Gen("231 text rows", base.but(text_len=231), oracle=True),
            Gen("77 text rows again", base, oracle=True)]
    outs = run_scenario(dev, "context length", gens, pipe)
    assert torch.equal(outs[2], outs[0]), "77 text rows after 231 differ from the first generation"
    assert not any(_long_layers(pipe.unet)) and pipe.unet._ctx.n_txt == 77


def test_rows_beyond_the_cap_are_refused_on_the_host(dev):
    from consistentid_amd import ops
    unet = new_unet(str(dev))
    cap = ops.xattn_long_max_txt()
    dc = unet.W[f"{next(iter(unet.packed.xattn_layers))}.attn2.kv_txt.w"].shape[1]
    with pytest.raises(ValueError, match=f"at most {cap} text rows"):
        unet.set_context(torch.zeros(2, cap + 1 + unet.num_tokens, dc, dtype=torch.float16, device=dev))
    unet.set_context(torch.zeros(2, 81, dc, dtype=torch.float16, device=dev))      # (nothing was left half-changed)


def test_a_controlnet_takes_the_cap_with_the_id_rows(dev):
    """a prompt of 1024 text rows reaches the ControlNet as 1024 + 4 rows of ONE text stream (``num_tokens=0``): it was refused
    there with the text cap.  Without ID rows the stream may fill the ID tile's slots too (33 key tiles either way)."""
    from consistentid_amd import ops
    net = new_net(str(dev), "A")
    cap, dc = ops.xattn_long_max_txt(), net.config.cross_attention_dim
    ehs = torch.randn(2, cap + 4, dc, generator=torch.Generator().manual_seed(0)).half().to(dev)
    net.set_context(ehs, num_tokens=0)
    assert (net._ctx.n_txt, net._ctx.n_ip) == (cap + 4, 0) and all(_long_layers(net))
    net.set_context(ehs[:, :4].repeat(1, (cap + 32) // 4, 1), num_tokens=0)
    assert net._ctx.n_txt == cap + ops.XATTN_LONG_MAX_IP
    with pytest.raises(ValueError, match=f"at most {cap + 32} text rows"):
        net.set_context(torch.zeros(2, cap + 33, dc, dtype=torch.float16, device=dev), num_tokens=0)
    assert net._ctx.n_txt == cap + 32                   # (nothing was left half-changed)


# ------------------------------------------------------------------------------------------------ encode_prompt
class _Tok(FakeTokenizer):
    pad_token_id = FakeTokenizer.eos_token_id       # CLIP-L pads with the end-of-text id


def _words(n, start=0):
    return " ".join(f"w{start + k}" for k in range(n))


@pytest.fixture(scope="module")
def tower(dev):
    from test_gpu_clip_text import _pair
    _, _, hip = _pair(dev, "tiny", False, eos=_Tok.eos_token_id, vocab=1024)
    return hip


def _chunk_outputs(tok, tower, dev, text):
    """the tower's fp16 outputs on the chunk ids of ``text`` as the restatement builds them -> ([77 m, Dc] fp16, weights, m)"""
    ids, ws = lpw_ref.stream(tok, text, 3)
    m = lpw_ref.multiple([(ids, ws)], 3)
    pi, pws = lpw_ref.padded(tok, ids, ws, m)
    rows = torch.tensor(lpw_ref.chunks(tok, pi, m), dtype=torch.long, device=dev)
    out = tower(rows)[0]
    assert out.dtype == torch.float16 and tuple(out.shape)[:2] == (m, 77)
    return out.reshape(77 * m, -1), lpw_ref.weights_per_position(pws, m), m


def test_encode_prompt_unweighted_long_is_the_chunks_concatenated(dev, tower):
    from consistentid_amd import prompt_encode
    tok = _Tok()
    text = _words(160)
    pos, neg = prompt_encode.encode_prompt(tok, tower, text, dev, do_classifier_free_guidance=False, max_embeddings_multiples=3)
    want, _, m = _chunk_outputs(tok, tower, dev, text)
    assert neg is None and m == 3 and pos.dtype == torch.float16 and tuple(pos.shape) == (1, 231, want.shape[-1])
    assert torch.equal(pos[0], want), f"max |diff| {(pos[0].float() - want.float()).abs().max():.3e}"


def test_encode_prompt_weighted_is_the_fp32_formula(dev, tower):
    """emb * w, rescaled by (mean before) / (mean after), in fp32 on the tower's fp16 outputs, rounded to fp16 once.  The
    product sums its means in another order than this test, so the fp32 values may differ in their last bits and the fp16
    result by one rounding step: |got - want| <= 2^-10 |want| (one fp16 ulp), plus half a subnormal step."""
    from consistentid_amd import prompt_encode
    tok = _Tok()
    text = "a (((portrait:1.3)) of [a] woman, (" + _words(100) + "), (sharp:0.7) focus, " + _words(40, 100)
    negative = "((((ugly)))), [out of frame]"
    pos, neg = prompt_encode.encode_prompt(tok, tower, text, dev, negative_prompt=negative, max_embeddings_multiples=3)
    for got, t in ((pos, text), (neg, negative)):
        out, w, m = _chunk_outputs(tok, tower, dev, t)
        if t is negative:         # the negative prompt is continued to the prompt's multiple
            assert m == 1
            ids, ws = lpw_ref.stream(tok, t, 3)
            pi, pws = lpw_ref.padded(tok, ids, ws, 2)
            out = tower(torch.tensor(lpw_ref.chunks(tok, pi, 2), dtype=torch.long, device=dev))[0].reshape(154, -1)
            w = lpw_ref.weights_per_position(pws, 2)
        e = out.float().cpu()
        ew = e * torch.tensor(w, dtype=torch.float32)[:, None]
        want = ew * (e.mean() / ew.mean())
        assert tuple(got.shape) == (1, 154, e.shape[-1]) and got.dtype == torch.float16
        err = (got[0].float().cpu() - want).abs()
        bound = want.abs() * 2.0 ** -10 + 2.0 ** -25
        print(f"[lpw] weighted encode: max |diff| {float(err.max()):.3e}, max of diff / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        assert float((got[0].float().cpu() - e).abs().max()) > 1e-2, "the weights changed nothing"
