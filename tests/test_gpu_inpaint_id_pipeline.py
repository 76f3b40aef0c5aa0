"""The reference's own call on the two inpaint pipelines, ``pipe(prompt, input_id_images=face, mask_image=<PIL>, height=,
width=, ...)`` (+ a PIL ``control_image``), on tiny models: every comparison is bit for bit against the explicit call that
gets the same tensors by hand (``prepare_id_prompt_embeds`` + image_prep.py), which tests/test_gpu_vae_encode.py,
tests/test_gpu_id_pipeline.py and tests/test_gpu_unet.py hold to the oracle.  No kernel is new on this path; the new code is
the host path that feeds the launches."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from test_gpu_id_pipeline import StubFaceApp, _face, tiny  # noqa: F401  (tiny: the module-scoped fixture, built here again)

pytestmark = pytest.mark.gpu

PROMPT = "a photo of a man"
H, W = 128, 192                                                  # 16 x 24 latents: a transposed size cannot pass
RUN = dict(num_inference_steps=2, output_type="latent", start_merge_step=0)
SIZE = dict(height=H, width=W)


def _gen(seed=7):
    return torch.Generator().manual_seed(seed)


def _mask():
    """PIL "L", 200 wide x 160 high: a filled rectangle and a band of noise, so that resampling and binarisation both matter"""
    a = np.zeros((160, 200), np.uint8)
    a[40:120, 60:150] = 255
    a[100:140] = np.random.default_rng(3).integers(0, 256, (40, 200), dtype=np.uint8)
    return Image.fromarray(a, "L")


def _control():
    return Image.fromarray(np.random.default_rng(4).integers(0, 256, (90, 100, 3), dtype=np.uint8), "RGB")


def _repeat_thirds(pe, n):
    return torch.cat([rows.repeat(n, 1, 1) for rows in pe.chunk(3)])


@pytest.fixture(scope="module")
def env(tiny, dev):
    """The three inpaint pipelines (4-channel, 9-channel, ControlNet) on their own tiny UNets, sharing the text tower, the
    small VAE encoder and the tiny ControlNet; the SD1.5 pipeline of ``tiny``; the inputs; and the 4-channel case's result,
    which several tests compare against."""
    from consistentid_amd import image_prep, pipeline, synth, unet_spec
    from consistentid_amd.unet import HipUNet
    from test_gpu_controlnet import _controlnet_pair
    from test_gpu_vae_encode import _vae
    h_vae = _vae(dev, "small")[2]
    h_cn = _controlnet_pair(dev)[2]
    ckpt_ids = {k: tiny.ckpt[k] for k in ("image_proj", "FacialEncoder")}

    def build(cls, in_channels=4, **kw):
        cfg = dataclasses.replace(unet_spec.tiny_config("sd15"), in_channels=in_channels)
        sd = synth.random_unet_state_dict(cfg, seed=0)
        ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=1)
        pipe = cls(HipUNet(cfg, sd, None, device=dev, keep_base=True), vae_encoder=h_vae,
                   text_encoder=tiny.pipe.text_encoder, tokenizer=tiny.pipe.tokenizer, **kw)
        return pipe.load_ConsistentID_model(dict(ckpt_ids, adapter_modules=ad), lora_rank=8,
                                            image_encoder_path=str(tiny.root / "clip_vision"),
                                            bise_net_cp=str(tiny.root / "face_parsing.pth"), face_app=StubFaceApp())

    e = SimpleNamespace(
        four=build(pipeline.StableDiffusionInpaintConsistentIDPipeline),
        nine=build(pipeline.StableDiffusionInpaintConsistentIDPipeline, in_channels=9),
        cn=build(pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline, controlnet=h_cn),
        t2i=tiny.pipe.load_ConsistentID_model(tiny.ckpt, lora_rank=8, image_encoder_path=str(tiny.root / "clip_vision"),
                                              bise_net_cp=str(tiny.root / "face_parsing.pth"), face_app=StubFaceApp()),
        face=_face(), mask=_mask())
    assert e.face.size == (300, 260) and e.mask.size == (200, 160)
    e.img_t = image_prep.preprocess_image(e.face, H, W)
    e.mask_t = image_prep.preprocess_mask(e.mask, H, W)
    assert tuple(e.img_t.shape) == (1, 3, H, W) and tuple(e.mask_t.shape) == (1, 1, H, W)
    assert 0.1 < float(e.mask_t.mean()) < 0.9
    e.pe = e.four.prepare_id_prompt_embeds(PROMPT, [e.face])
    e.four_out = e.four(PROMPT, input_id_images=e.face, mask_image=e.mask, generator=_gen(), **SIZE, **RUN).images
    torch.cuda.synchronize()
    return e


def test_four_channel_call_is_the_explicit_call(env):
    a, pipe = env.four_out, env.four
    assert tuple(a.shape) == (1, 4, H // 8, W // 8) and torch.isfinite(a.float()).all()
    b = pipe(prompt_embeds=env.pe, image=env.img_t, mask_image=env.mask_t, generator=_gen(), **RUN).images
    assert torch.equal(a, b)
    c = pipe(PROMPT, input_id_images=[env.face], mask_image=env.mask, generator=_gen(), **SIZE, **RUN).images
    assert torch.equal(a, c)


def test_nine_channel_call_is_the_explicit_call(env):
    pipe = env.nine
    a = pipe(PROMPT, input_id_images=env.face, mask_image=env.mask, strength=0.6, generator=_gen(), **SIZE, **RUN).images
    pe = pipe.prepare_id_prompt_embeds(PROMPT, [env.face])
    b = pipe(prompt_embeds=pe, image=env.img_t, mask_image=env.mask_t, strength=0.6, generator=_gen(), **RUN).images
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 4, H // 8, W // 8) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    c = pipe(PROMPT, input_id_images=[env.face], mask_image=env.mask, strength=0.6, generator=_gen(), **SIZE, **RUN).images
    assert torch.equal(a, c)


def test_controlnet_call_with_pil_control_image(env):
    from consistentid_amd import image_prep
    pipe, ctrl = env.cn, _control()
    assert ctrl.size == (100, 90)
    cn_kw = dict(controlnet_conditioning_scale=0.5, **RUN)
    a = pipe(PROMPT, input_id_images=env.face, mask_image=env.mask, control_image=ctrl, generator=_gen(), **SIZE,
             **cn_kw).images
    pe = pipe.prepare_id_prompt_embeds(PROMPT, [env.face])
    ctrl_t = image_prep.preprocess_control(ctrl, H, W)
    assert tuple(ctrl_t.shape) == (1, 3, H, W)
    b = pipe(prompt_embeds=pe, image=env.img_t, mask_image=env.mask_t, control_image=ctrl_t, generator=_gen(), **cn_kw).images
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 4, H // 8, W // 8) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    c = pipe(PROMPT, input_id_images=env.face, mask_image=env.mask, control_image=[ctrl], generator=_gen(), **SIZE,
             **cn_kw).images
    assert torch.equal(a, c)
    assert not torch.equal(a, env.four_out)                      # the same weights without the ControlNet
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        pipe(PROMPT, input_id_images=env.face, mask_image=env.mask, control_image=[ctrl, ctrl], generator=_gen(), **SIZE,
             **cn_kw)


def test_image_argument_takes_precedence_as_init_image(env):
    from consistentid_amd import image_prep
    pipe, other = env.four, _face(seed=205)
    a = pipe(PROMPT, input_id_images=env.face, image=other, mask_image=env.mask, generator=_gen(), **SIZE, **RUN).images
    b = pipe(prompt_embeds=env.pe, image=image_prep.preprocess_image(other, H, W), mask_image=env.mask_t, generator=_gen(),
             **RUN).images
    assert torch.equal(a, b)
    assert not torch.equal(a, env.four_out)


def test_num_images_per_prompt(env, dev):
    from consistentid_amd.vae import randn_tensor
    h, w = H // 8, W // 8
    a = env.four(PROMPT, input_id_images=env.face, mask_image=env.mask, num_images_per_prompt=2, generator=_gen(), **SIZE,
                 **RUN).images
    b = env.four(prompt_embeds=_repeat_thirds(env.pe, 2), image=env.img_t, mask_image=env.mask_t, generator=_gen(),
                 **RUN).images
    assert tuple(a.shape) == (2, 4, h, w) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    assert not torch.equal(a[0], a[1])
    # the text-to-image pipeline: the latents are one draw of [2, C, h, w] on the generator
    t2i = env.t2i
    a = t2i(PROMPT, input_id_images=[env.face], num_images_per_prompt=2, generator=_gen(5), **SIZE, **RUN).images
    pe = t2i.prepare_id_prompt_embeds(PROMPT, [env.face])
    lat = randn_tensor((2, 4, h, w), generator=_gen(5), device=dev, dtype=torch.float16)
    b = t2i(prompt_embeds=_repeat_thirds(pe, 2), latents=lat, **RUN).images
    torch.cuda.synchronize()
    assert tuple(a.shape) == (2, 4, h, w) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    assert not torch.equal(a[0], a[1])
    with pytest.raises(ValueError, match="num_images_per_prompt"):
        t2i(PROMPT, input_id_images=[env.face], num_images_per_prompt=0, **SIZE, **RUN)
    with pytest.raises(ValueError, match="num_images_per_prompt"):
        t2i(PROMPT, input_id_images=[env.face], num_images_per_prompt=2, latents=lat[:1], **RUN)


def test_refusals(env, monkeypatch):
    from consistentid_amd import pipeline
    pipe = env.four
    call = dict(mask_image=env.mask, generator=_gen(), **SIZE, **RUN)
    with pytest.raises(ValueError, match="go together"):
        pipe(PROMPT, **call)
    with pytest.raises(ValueError, match="go together"):
        pipe(input_id_images=env.face, **call)
    with pytest.raises(ValueError, match="not both"):
        pipe(PROMPT, input_id_images=env.face, prompt_embeds=env.pe, **call)
    with pytest.raises(NotImplementedError):
        pipe(PROMPT, input_id_images=env.face, **dict(call, mask_image=np.zeros((H, W), np.float32)))
    with pytest.raises(NotImplementedError):
        pipe(prompt_embeds=env.pe, image=env.img_t, mask_image=env.mask_t.numpy(), generator=_gen(), **RUN)
    with pytest.raises(ValueError, match="not resized"):       # float tensors keep their behaviour: no resizing
        pipe(prompt_embeds=env.pe, image=env.img_t, mask_image=env.mask_t, generator=_gen(), height=64, **RUN)
    with pytest.raises(TypeError):                               # the plain inpaint pipeline takes no control_image
        pipe(PROMPT, input_id_images=env.face, control_image=_control(), **call)
    sdxl = pipeline.ConsistentIDStableDiffusionXLPipeline(pipe.unet)
    with pytest.raises(NotImplementedError, match="SD1.5 pipeline only"):
        sdxl(prompt=PROMPT, input_id_images=env.face, output_type="latent")
    monkeypatch.setattr(pipe, "app", None)
    with pytest.raises(NotImplementedError, match="FaceID app"):
        pipe(PROMPT, input_id_images=env.face, **call)
