"""The SD1.5 pipeline's ID pre-loop end to end on tiny models: ``pipe(prompt, input_id_images=[face])`` with a stub FaceID
app, HipBiSeNet face parsing, a tiny transformers CLIP vision tower and a tiny ConsistentID checkpoint, against an
independent composition (fp32 BiSeNet restatement, the host mask / crop code, transformers' CLIP vision, oracle/idstack.py);
plus the ReLU epilogue with a second destination and a time row."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bisenet_ref import calibrate, forward, make_image, random_state_dict
from conftest import check_close

pytestmark = pytest.mark.gpu


class StubFaceApp:
    """insightface FaceAnalysis' interface as the reference uses it: get(RGB array) -> faces with normed_embedding"""

    def __init__(self, faces=True):
        self.faces, self.calls = faces, 0
        e = np.random.default_rng(0).standard_normal(512).astype(np.float32)
        self.emb = e / np.linalg.norm(e)

    def get(self, arr):
        assert isinstance(arr, np.ndarray) and arr.ndim == 3 and arr.shape[-1] == 3
        self.calls += 1
        return [SimpleNamespace(normed_embedding=self.emb)] if self.faces else []


@pytest.fixture(scope="module")
def tiny(tmp_path_factory, dev):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from consistentid_amd import pipeline, synth, unet_spec
    from oracle import idstack
    from oracle_utils import idstack_weights
    from test_clip_text_host import make_tokenizer_dir, tiny_text_config
    from test_gpu_clip_text import _save_tower
    from test_loader import _write_component
    root = tmp_path_factory.mktemp("idpipe")
    cfg = unet_spec.tiny_config("sd15")
    sd = synth.random_unet_state_dict(cfg, seed=0)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=1)
    _write_component(root / "base" / "unet", {"block_out_channels": list(cfg.block_out_channels),
                                              "down_block_types": list(cfg.down_block_types),
                                              "up_block_types": list(cfg.up_block_types), "layers_per_block": 1,
                                              "attention_head_dim": 2, "cross_attention_dim": 128, "sample_size": 32},
                     sd, "safetensors")
    V = make_tokenizer_dir(root / "base" / "tokenizer")
    text_ref = _save_tower(root / "base" / "text_encoder", tiny_text_config(V, eos_token_id=2), False, seed=7)
    vcfg = CLIPVisionConfig(hidden_size=192, intermediate_size=384, num_hidden_layers=2, num_attention_heads=3,
                            image_size=224, patch_size=14, projection_dim=64, hidden_act="gelu")
    torch.manual_seed(3)
    vis_ref = CLIPVisionModelWithProjection(vcfg).eval()
    with torch.no_grad():
        for p in vis_ref.parameters():
            p.copy_(p.half().float())
    vis_ref.save_pretrained(str(root / "clip_vision"))
    bise = random_state_dict(seed=11)
    calibrate(bise, make_image(1, 512, 512, seed=100))
    torch.save(bise, str(root / "face_parsing.pth"))
    o_ip = idstack.ProjPlusModel(cross_attention_dim=128, id_embeddings_dim=512, clip_embeddings_dim=192)
    o_fe = idstack.FacialEncoder(embedding_dim=192, output_dim=128, embed_dim=128)
    sd_ip, sd_fe = idstack_weights(o_ip, 3), idstack_weights(o_fe, 4)
    o_ip.load_state_dict(sd_ip)
    o_fe.load_state_dict(sd_fe)
    ckpt = {"adapter_modules": ad, "image_proj": sd_ip, "FacialEncoder": sd_fe}
    pipe = pipeline.ConsistentIDStableDiffusionPipeline.from_pretrained(str(root / "base"), device=dev)
    return SimpleNamespace(root=root, pipe=pipe, ckpt=ckpt, text_ref=text_ref, vis_ref=vis_ref, bise=bise,
                           o_ip=o_ip.eval(), o_fe=o_fe.eval())


def _face(seed=201):
    from PIL import Image
    return Image.fromarray(make_image(1, 260, 300, seed=seed)[0].numpy())


def _load(t, face_app):
    return t.pipe.load_ConsistentID_model(t.ckpt, lora_rank=8, image_encoder_path=str(t.root / "clip_vision"),
                                          bise_net_cp=str(t.root / "face_parsing.pth"), face_app=face_app)


def test_refusals_name_the_missing_component(tiny):
    pipe = tiny.pipe
    pipe.load_ConsistentID_model(tiny.ckpt, lora_rank=8)
    with pytest.raises(NotImplementedError, match="FaceID app.*BiSeNet.*image encoder"):
        pipe(prompt="a photo of a man", input_id_images=[object()])
    with pytest.raises(FileNotFoundError, match="bise_net_cp"):
        pipe.load_ConsistentID_model(tiny.ckpt, lora_rank=8, bise_net_cp=str(tiny.root / "nope.pth"))
    with pytest.raises(FileNotFoundError, match="image_encoder_path"):
        pipe.load_ConsistentID_model(tiny.ckpt, lora_rank=8, image_encoder_path=str(tiny.root / "nope"))
    _load(tiny, None)
    with pytest.raises(NotImplementedError, match="FaceID app") as e:
        pipe(prompt="a photo of a man", input_id_images=[object()])
    assert "BiSeNet" not in str(e.value)


def test_prepare_id_prompt_embeds_matches_independent_composition(tiny, dev):
    from consistentid_amd import face_prep
    from consistentid_amd.face_parsing import to_pixels
    from consistentid_amd.prompt_utils import encode_prompt_with_trigger_word
    from oracle import idstack
    from test_gpu_clip_text import _diffusers_encode
    app = StubFaceApp()
    pipe = _load(tiny, app)
    assert pipe.app is app
    img, prompt = _face(), "a photo of a man"
    got = pipe.prepare_id_prompt_embeds(prompt, [img])
    torch.cuda.synchronize()
    assert got.shape == (3, 81, 128) and torch.isfinite(got.float()).all()
    # the independent composition: fp32 BiSeNet restatement -> host masks / crops -> transformers CLIP -> oracle ID stack
    labels = forward(tiny.bise, to_pixels(img)).argmax(1)[0].numpy().astype(np.uint8)
    hip_labels = pipe.parsing_face_mask(img)[1]
    print(f"[id pipeline] label agreement {float((labels == hip_labels).mean()):.5f}")
    masks = face_prep.select_face_masks(face_prep.masks_for_unique_values(labels))
    assert list(masks) == list(pipe.get_prepare_facemask(img)[0])
    caption = pipe.get_prepare_llva_caption(img)
    text_only, clean_ids, masks_align, fmask, _, fidx_mask = encode_prompt_with_trigger_word(
        pipe.tokenizer, prompt, caption, masks, max_num_facials=5, num_id_images=1)
    tok, tref = pipe.tokenizer, tiny.text_ref
    with torch.no_grad():
        text_embeds = tref(clean_ids)[0]
        pos, neg = _diffusers_encode(tok, tref, [text_only]), _diffusers_encode(tok, tref, [""])
        pix = lambda im: torch.from_numpy(face_prep.clip_preprocess(im))[None]
        hs = lambda x: tiny.vis_ref(x, output_hidden_states=True).hidden_states[-2]
        face_hs, zero_hs = hs(pix(img)), hs(torch.zeros(1, 3, 224, 224))
        crops = [hs(pix(face_prep.fetch_mask_raw_image(img, m))) for m in masks_align.values()]
        facial = torch.cat(crops + [zero_hs] * (5 - len(crops)))[None]
        ref = idstack.assemble_prompt_embeds(
            tiny.o_ip, tiny.o_fe, text_embeds=text_embeds, negative_embeds=neg, text_only_embeds=pos,
            faceid_embeds=torch.from_numpy(app.emb)[None], clip_embeds=face_hs, uncond_clip_embeds=zero_hs,
            facial_embeds=facial, uncond_facial_embeds=zero_hs.expand(5, *zero_hs.shape[1:])[None],
            facial_token_mask=fmask, valid_facial_mask=fidx_mask)
    check_close(got, ref, "prepare_id_prompt_embeds vs the independent composition", tol_l2=2e-2, tol_max=0.25)
    # the reference's per-method return values
    fid = pipe.get_prepare_faceid(img)
    assert fid.shape == (1, 512) and torch.equal(fid[0], torch.from_numpy(app.emb))
    clip_img, fmasks = pipe.get_prepare_clip_image(img, masks_align)
    assert clip_img.shape == (5, 3, 224, 224) and fmasks.shape == (5, 512, 512)
    assert clip_img[len(masks_align):].abs().sum() == 0 and fmasks[len(masks_align):].abs().sum() == 0
    overlay, lab = pipe.parsing_face_mask(img)
    assert overlay.shape == (512, 512, 3) and overlay.dtype == np.uint8 and lab.shape == (512, 512)


def test_call_with_input_id_images_is_the_same_as_prompt_embeds(tiny, dev):
    from consistentid_amd.vae import randn_tensor
    pipe = _load(tiny, StubFaceApp())
    img, prompt = _face(seed=202), "a photo of a woman"
    a = pipe(prompt, input_id_images=[img], generator=torch.Generator().manual_seed(5), num_inference_steps=2,
             output_type="latent").images
    pe = pipe.prepare_id_prompt_embeds(prompt, [img])
    lat = randn_tensor((1, 4, 32, 32), generator=torch.Generator().manual_seed(5), device=dev, dtype=torch.float16)
    b = pipe(prompt_embeds=pe, latents=lat, num_inference_steps=2, output_type="latent").images
    torch.cuda.synchronize()
    assert a.shape == (1, 4, 32, 32) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    c = pipe(prompt, input_id_images=img, latents=lat, num_inference_steps=2, output_type="latent").images    # one PIL image
    assert torch.equal(a, c)
    with pytest.raises(ValueError, match="not both"):
        pipe(prompt, input_id_images=[img], prompt_embeds=pe, latents=lat, output_type="latent")


def test_no_face_gives_zero_faceid_embeds(tiny, dev):
    pipe = _load(tiny, StubFaceApp(faces=False))
    img = _face(seed=203)
    fid = pipe.get_prepare_faceid(img)
    assert fid.shape == (1, 512) and fid.abs().sum() == 0
    pe = pipe.prepare_id_prompt_embeds("a photo of a man", [img])
    torch.cuda.synchronize()
    assert torch.isfinite(pe.float()).all()
    # the FaceID tokens of the conditional and the unconditional rows now come from the same zero embedding; they differ only
    # through the CLIP input (the face image vs a zero image)
    tok, utok = pipe.get_image_embeds(fid, img, s_scale=1.0)
    assert tok.shape == utok.shape == (1, 4, 128)


def test_gemm_act_with_out2_and_rowbias(dev):
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(3)
    B, HW, cin, cout = 2, 1024, 128, 320
    x = torch.randn(B * HW, cin, generator=g).half()
    w = (torch.randn(cout, cin, generator=g) * cin ** -0.5).half()
    rb = (torch.randn(B, cout, generator=g)).half()
    ref = torch.relu(x.float() @ w.float().T + rb.float().repeat_interleave(HW, 0))
    outs = []
    for act in (0, 1):
        out = torch.full((B * HW, cout), float("nan"), dtype=torch.float16, device=dev)
        out2 = torch.full_like(out, float("nan"))
        ops.gemm(x.to(dev), w.to(dev), out, M=B * HW, N=cout, c1=cin, rowbias=rb.to(dev), ld_rowbias=cout,
                 rows_per_sample=HW, out2=out2, act=act)
        outs.append((out, out2))
    torch.cuda.synchronize()
    (p, p2), (r, r2) = [(a.cpu(), b.cpu()) for a, b in outs]
    assert torch.equal(p, p2) and torch.equal(r, r2)
    assert torch.equal(r, torch.relu(p)) and (p < 0).any()
    check_close(r, ref, "act 1 with rowbias and out2", tol_l2=2e-3, tol_max=2e-2)
