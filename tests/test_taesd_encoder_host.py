"""AutoencoderTiny's encoder on the host: the layer walk, weight packing, the config / state-dict refusals, the loader's
dispatch and both ``from_pretrained`` paths, the ABI and the argument checks of the ops wrappers.  No GPU: the engine is never
built here (its constructor moves the packed weights to the device); everything it decides on the host is a pure function of
vae_tiny."""
import json
import os

import pytest
import torch

import taesd_enc_ref as E
import taesd_ref as R


@pytest.fixture(scope="module")
def model():
    return E.synthetic(3)


@pytest.fixture(scope="module")
def sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ----------------------------------------------------------------------------- packing
def test_layer_walk_of_the_published_encoder():
    from consistentid_amd.vae_tiny import tiny_encoder_layers
    assert tiny_encoder_layers((1, 3, 3, 3)) == [
        ("in", 0), ("block", 1), ("down", 2), ("block", 3), ("block", 4), ("block", 5), ("down", 6), ("block", 7), ("block", 8),
        ("block", 9), ("down", 10), ("block", 11), ("block", 12), ("block", 13), ("out", 14)]
    assert tiny_encoder_layers((1, 2)) == [("in", 0), ("block", 1), ("down", 2), ("block", 3), ("block", 4), ("out", 5)]
    assert tiny_encoder_layers((2,)) == [("in", 0), ("block", 1), ("block", 2), ("out", 3)]


def test_reference_has_the_published_keys(sd):
    """the restatement itself: 15 layers, biases where diffusers has them"""
    idx = {int(k.split(".")[2]) for k in sd}
    assert idx == set(range(15))
    assert sd["encoder.layers.0.weight"].shape == (64, 3, 3, 3) and sd["encoder.layers.14.weight"].shape == (4, 64, 3, 3)
    for i in (2, 6, 10):
        assert f"encoder.layers.{i}.weight" in sd and f"encoder.layers.{i}.bias" not in sd


def test_packing_maps_diffusers_keys(sd):
    from consistentid_amd.vae_tiny import pack_tiny_encoder
    walk, packed = pack_tiny_encoder(E.config(), sd)
    assert walk[-1] == ("out", 14)
    for k, t in packed.items():
        assert t.dtype == torch.float16 and t.is_contiguous(), k
    assert packed["0.w"].shape == (64, 9, 3) and packed["0.b"].shape == (64,)
    assert packed["14.w"].shape == (4, 9, 64) and packed["14.b"].shape == (4,)
    for i in (1, 3, 4, 5, 7, 8, 9, 11, 12, 13):
        for j in (0, 2, 4):
            assert packed[f"{i}.{j}.w"].shape == (64, 9, 64) and packed[f"{i}.{j}.b"].shape == (64,)
            assert torch.equal(packed[f"{i}.{j}.b"].float(), sd[f"encoder.layers.{i}.conv.{j}.bias"])
    for i in (2, 6, 10):                                          # the stride-2 convs carry no bias
        assert packed[f"{i}.w"].shape == (64, 9, 64) and f"{i}.b" not in packed
    assert torch.equal(packed["0.b"].float(), sd["encoder.layers.0.bias"])
    assert torch.equal(packed["14.b"].float(), sd["encoder.layers.14.bias"])
    assert len(packed) == 2 + 10 * 6 + 3 + 2
    # one tap of one layer against the torch weight: tap = 3 ky + kx, [cout][tap][cin]
    w = sd["encoder.layers.8.conv.2.weight"]
    ky, kx = 2, 0
    assert torch.equal(packed["8.2.w"][:, 3 * ky + kx, :].float(), w[:, :, ky, kx])
    assert float(packed["8.2.w"][5, 7, 11]) == float(w[5, 11, 2, 1])
    assert torch.equal(packed["0.w"][:, 1, :].float(), sd["encoder.layers.0.weight"][:, :, 0, 1])
    assert torch.equal(packed["6.w"][:, 5, :].float(), sd["encoder.layers.6.weight"][:, :, 1, 2])
    assert torch.equal(packed["14.w"][:, 8, :].float(), sd["encoder.layers.14.weight"][:, :, 2, 2])


def test_packing_ignores_the_decoder_and_takes_other_block_counts(sd):
    from consistentid_amd.vae_tiny import pack_tiny_encoder
    whole = dict(sd)
    whole.update(R.synthetic(0).state_dict())
    assert any(k.startswith("decoder.") for k in whole)
    assert set(pack_tiny_encoder(E.config(), whole)[1]) == set(pack_tiny_encoder(E.config(), sd)[1])
    small = E.synthetic(1, (1, 2))
    walk, packed = pack_tiny_encoder(E.config((1, 2)), small.state_dict())
    assert walk[-1] == ("out", 5) and "2.w" in packed and "2.b" not in packed and packed["5.w"].shape == (4, 9, 64)


# ----------------------------------------------------------------------------- refusals
class Untouchable(dict):
    """a state dict that must not be read: the config is refused before any weight is touched"""
    def __getitem__(self, k):
        raise AssertionError(f"weight {k} was read before the config was checked")

    def __iter__(self):
        raise AssertionError("the state dict was walked before the config was checked")


@pytest.mark.parametrize("key,value", [("act_fn", "swish"), ("encoder_block_out_channels", [64, 64, 128, 64]),
                                       ("encoder_block_out_channels", [64, 64, 64]), ("block_out_channels", [64, 32, 64, 64]),
                                       ("block_out_channels", [64] * 5), ("in_channels", 4), ("latent_channels", 16),
                                       ("num_encoder_blocks", [1, 0, 3, 3]), ("num_encoder_blocks", [])])
def test_config_refusals_name_the_key(key, value):
    from consistentid_amd.vae_tiny import HipAutoencoderTinyEncoder, check_tiny_encoder_config, pack_tiny_encoder
    cfg = E.config()
    cfg[key] = value
    with pytest.raises(NotImplementedError, match=key):
        check_tiny_encoder_config(cfg)
    with pytest.raises(NotImplementedError, match=key):
        pack_tiny_encoder(cfg, Untouchable())
    with pytest.raises(NotImplementedError, match=key):
        HipAutoencoderTinyEncoder(cfg, Untouchable(), device="cpu")


def test_config_accepts_any_positive_block_counts():
    from consistentid_amd.vae_tiny import check_tiny_encoder_config
    assert check_tiny_encoder_config(E.config()) == (1, 3, 3, 3)
    assert check_tiny_encoder_config(E.config((2, 5))) == (2, 5)
    assert check_tiny_encoder_config({}) == (1, 3, 3, 3)          # diffusers' defaults


def test_layer_list_that_does_not_match_num_encoder_blocks(sd):
    from consistentid_amd.vae_tiny import pack_tiny_encoder
    with pytest.raises(NotImplementedError, match="num_encoder_blocks"):
        pack_tiny_encoder(E.config((1, 3, 3, 4)), sd)              # one Block more than the weights have
    with pytest.raises(NotImplementedError, match="num_encoder_blocks"):
        pack_tiny_encoder(E.config((1, 3, 3)), sd)


def test_missing_and_unexpected_encoder_keys(sd):
    from consistentid_amd.vae_tiny import pack_tiny_encoder
    gone = {k: v for k, v in sd.items() if k != "encoder.layers.9.conv.2.bias"}
    with pytest.raises(NotImplementedError, match=r"encoder\.layers\.9\.conv\.2\.bias"):
        pack_tiny_encoder(E.config(), gone)
    extra = dict(sd)
    extra["encoder.layers.6.bias"] = torch.zeros(64)                # the stride-2 conv has no bias
    with pytest.raises(NotImplementedError, match=r"encoder\.layers\.6\.bias"):
        pack_tiny_encoder(E.config(), extra)
    skip = dict(sd)
    skip["encoder.layers.3.skip.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(NotImplementedError, match=r"encoder\.layers\.3\.skip\.weight"):
        pack_tiny_encoder(E.config(), skip)
    shape = dict(sd)
    shape["encoder.layers.0.weight"] = torch.zeros(64, 4, 3, 3)
    with pytest.raises(NotImplementedError, match=r"encoder\.layers\.0\.weight"):
        pack_tiny_encoder(E.config(), shape)
    # a Block where the walk has a stride-2 conv: same count of layers, other keys
    moved = {k.replace("layers.2.", "layers.2.conv.0."): v for k, v in sd.items()}
    with pytest.raises(NotImplementedError, match=r"encoder\.layers\.2\."):
        pack_tiny_encoder(E.config(), moved)


def test_the_decoder_class_still_does_not_encode():
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    with pytest.raises(NotImplementedError, match="AutoencoderTiny.encode is not built") as e:
        HipAutoencoderTiny.encode(object.__new__(HipAutoencoderTiny), torch.zeros(1, 3, 8, 8))
    assert "HipAutoencoderTinyEncoder" in str(e.value)


def test_exported_from_the_package():
    import consistentid_amd
    from consistentid_amd.vae_tiny import HipAutoencoderTinyEncoder
    assert consistentid_amd.HipAutoencoderTinyEncoder is HipAutoencoderTinyEncoder
    assert "HipAutoencoderTinyEncoder" in consistentid_amd.__all__


def test_encode_inpaint_refusals_need_no_gpu(sd):
    """the size and downscale refusals of encode_inpaint come before any launch"""
    from consistentid_amd.vae_tiny import HipAutoencoderTinyEncoder
    enc = HipAutoencoderTinyEncoder(E.config(), sd, device="cpu")
    assert enc.downscale == 8 and enc.dtype == torch.float16 and enc.device == torch.device("cpu")
    assert enc.config.scaling_factor == 1.0 and enc.config.latent_channels == 4 and enc.config.in_channels == 3
    assert enc.config.force_upcast is False and enc.config.num_encoder_blocks == (1, 3, 3, 3)
    img, msk = torch.zeros(2, 3, 16, 24), torch.zeros(2, 1, 16, 24)
    with pytest.raises(ValueError, match="multiples of 8"):
        enc.encode_inpaint(img[..., :20], msk[..., :20])
    with pytest.raises(ValueError, match="mask must be"):
        enc.encode_inpaint(img, msk[..., :16])
    with pytest.raises(ValueError, match="mask must be"):
        enc.encode_inpaint(torch.zeros(3, 3, 16, 24), msk)
    with pytest.raises(ValueError, match="nothing to encode"):
        enc.encode_inpaint(img, msk, encode_image=False, encode_masked=False)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        enc.encode(torch.zeros(1, 4, 8, 8))
    small = HipAutoencoderTinyEncoder(E.config((1, 2)), E.synthetic(1, (1, 2)).state_dict(), device="cpu")
    assert small.downscale == 2
    with pytest.raises(ValueError, match="downsamples by 2"):
        small.encode_inpaint(img, msk)


# ----------------------------------------------------------------------------- loader
class _Built:
    """stands in for an engine class: records what the loader hands it (no GPU here)"""
    def __init__(self, *a, **kw):
        self.args, self.kw = a, kw


def _kl_folder(path):
    from consistentid_amd import synth, vae_spec
    from safetensors.torch import save_file
    vcfg = vae_spec.tiny_vae_config()
    os.makedirs(path)
    kl_cfg = {"_class_name": "AutoencoderKL", "in_channels": vcfg.in_channels, "out_channels": vcfg.out_channels,
              "latent_channels": vcfg.latent_channels, "block_out_channels": list(vcfg.block_out_channels),
              "layers_per_block": vcfg.layers_per_block, "norm_num_groups": vcfg.norm_num_groups,
              "scaling_factor": vcfg.scaling_factor, "force_upcast": vcfg.force_upcast}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(kl_cfg, f)
    save_file({k: v.cpu().contiguous() for k, v in synth.random_vae_state_dict(vcfg, seed=5, device="cpu").items()},
              os.path.join(path, "diffusion_pytorch_model.safetensors"))
    return kl_cfg


def test_load_tiny_vae_encoder(tmp_path, model, monkeypatch):
    from consistentid_amd import loader, vae_tiny
    tiny = type("TinyEnc", (_Built,), {})
    monkeypatch.setattr(vae_tiny, "HipAutoencoderTinyEncoder", tiny)
    E.write_folder(tmp_path / "taesd", model, extra=R.synthetic(0).state_dict())          # a whole AutoencoderTiny
    got = loader.load_tiny_vae_encoder(tmp_path / "taesd", device="cpu")
    assert type(got) is tiny and got.args[0]["_class_name"] == "AutoencoderTiny" and got.kw == {"device": "cpu"}
    assert "encoder.layers.14.bias" in got.args[1] and got.args[1]["encoder.layers.14.bias"].dtype == torch.float16
    # a decoder-only export is refused by name, and so is a KL folder
    R.write_folder(tmp_path / "decoder_only", R.synthetic(0))
    with pytest.raises(NotImplementedError, match=r"encoder\.\*"):
        loader.load_tiny_vae_encoder(tmp_path / "decoder_only", device="cpu")
    _kl_folder(tmp_path / "kl")
    with pytest.raises(NotImplementedError, match="AutoencoderKL"):
        loader.load_tiny_vae_encoder(tmp_path / "kl", device="cpu")


def test_from_pretrained_builds_the_encoder_by_class_name(tmp_path, model, monkeypatch):
    """the two inpaint pipelines get the tiny encoder from a tiny ``vae/`` folder that has encoder.* keys, the KL encoder from
    a KL folder, nothing from a decoder-only tiny folder; every other pipeline gets none; ``vae_encoder=`` replaces the
    folder's; junk is refused before anything is read"""
    from consistentid_amd import loader, pipeline, vae, vae_tiny
    tiny = type("TinyEnc", (_Built,), {"encode_inpaint": lambda self, *a, **k: None})
    kl = type("KLEnc", (_Built,), {"encode_inpaint": lambda self, *a, **k: None})
    monkeypatch.setattr(vae_tiny, "HipAutoencoderTinyEncoder", tiny)
    monkeypatch.setattr(vae, "HipVAEEncoder", kl)
    monkeypatch.setattr(loader, "load_unet", lambda root, device="cuda:0": "unet")
    monkeypatch.setattr(loader, "_make_decoder", lambda cfg, sd, device: ("folder decoder", cfg["_class_name"]))
    seen = {}

    def stand_in(base):
        class Pipe(base):
            def __init__(self, unet, **kw):
                seen.clear()
                seen.update(kw)
        return Pipe

    inpaint = stand_in(pipeline.StableDiffusionInpaintConsistentIDPipeline)
    cn_inpaint = stand_in(pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline)
    txt2img = stand_in(pipeline.ConsistentIDStableDiffusionPipeline)
    E.write_folder(tmp_path / "whole" / "vae", model, extra=R.synthetic(0).state_dict())
    R.write_folder(tmp_path / "decoder_only" / "vae", R.synthetic(0))
    kl_cfg = _kl_folder(tmp_path / "kl" / "vae")

    for cls in (inpaint, cn_inpaint):
        loader.from_pretrained(cls, tmp_path / "whole")
        assert type(seen["vae_encoder"]) is tiny and seen["vae"] == ("folder decoder", "AutoencoderTiny")
        assert seen["vae_encoder"].args[0]["_class_name"] == "AutoencoderTiny" and "encoder.layers.0.weight" in seen["vae_encoder"].args[1]
        loader.from_pretrained(cls, tmp_path / "kl")
        assert type(seen["vae_encoder"]) is kl and seen["vae_encoder"].args[0] == loader.vae_config_from_diffusers(kl_cfg)
        loader.from_pretrained(cls, tmp_path / "decoder_only")
        assert "vae_encoder" not in seen and seen["vae"] == ("folder decoder", "AutoencoderTiny")
    for root in ("whole", "kl", "decoder_only"):
        loader.from_pretrained(txt2img, tmp_path / root)
        assert "vae_encoder" not in seen
    # a built encoder replaces the folder's (neither class is constructed), also beside a built decoder
    mine = tiny()
    loader.from_pretrained(inpaint, tmp_path / "kl", vae_encoder=mine)
    assert seen["vae_encoder"] is mine and seen["vae"] == ("folder decoder", "AutoencoderKL")
    dec = _Built()
    dec.decode_latents = lambda x: x
    loader.from_pretrained(inpaint, tmp_path / "whole", vae=dec, vae_encoder=mine)
    assert seen["vae_encoder"] is mine and seen["vae"] is dec
    for junk in ("madebyollin/taesd", None, dec):
        with pytest.raises(TypeError, match="vae_encoder="):
            loader.from_pretrained(inpaint, tmp_path / "nowhere", vae_encoder=junk)


def test_pipeline_attribute_takes_either_encoder():
    """``vae_encoder=`` in the constructor and ``pipe.vae_encoder = ...`` are plain attributes; ``pipe.vae = ...`` leaves the
    encoder alone (no engine is built here: the base constructor is bypassed)"""
    from consistentid_amd import pipeline
    pipe = object.__new__(pipeline.StableDiffusionInpaintConsistentIDPipeline)
    a, b = _Built(), _Built()
    pipe.vae_encoder = a
    pipe.vae = b
    assert pipe.vae_encoder is a
    import inspect
    assert "vae_encoder" in inspect.signature(pipeline._BasePipeline.__init__).parameters


# ----------------------------------------------------------------------------- ABI and wrappers
def test_abi_exports_and_version(lib):
    for name in ("cid_tiny_conv64_s2_f16", "cid_tiny_conv64_s2_tile", "cid_tiny_encode_in_f16", "cid_tiny_encode_out_f16"):
        assert hasattr(lib, name), name
    assert lib.cid_version() >= 113
    from consistentid_amd import ops
    th, tw, cap = ops.tiny_conv64_s2_tile()
    assert th >= 1 and tw >= 1 and cap >= 1
    # the LDS arithmetic of the tile: the (2 th + 1) x (2 tw + 1) halo beside the 72 KiB weight fits 160 KiB
    assert (2 * th + 1) * (2 * tw + 1) * 128 + 9 * 64 * 128 <= 160 * 1024


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """-22 with a text, on a machine without a GPU: nothing is launched for a refused call"""
    a = 4096                                  # an aligned stand-in address: refused calls never dereference it
    assert lib.cid_tiny_conv64_s2_f16(None, a, a, 1, 4, 4, None) == -22
    assert b"null" in lib.cid_last_error()
    assert lib.cid_tiny_conv64_s2_f16(a, 2 * a, a, 1, 0, 4, None) == -22
    assert lib.cid_tiny_conv64_s2_f16(a, 2 * a, a, 0, 4, 4, None) == -22
    assert lib.cid_tiny_conv64_s2_f16(a, 2 * a + 8, a, 1, 4, 4, None) == -22
    assert b"aligned" in lib.cid_last_error()
    assert lib.cid_tiny_conv64_s2_f16(a, a, a + 64, 1, 4, 4, None) == -22
    assert b"alias" in lib.cid_last_error()
    assert lib.cid_tiny_encode_in_f16(None, 1, None, 0, a, a, a, 8, 8, 0, 1, None, None) == -22
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a, a, a, 8, 8, 0, 0, None, None) == -22
    assert b"blocks" in lib.cid_last_error()
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a, a, a, 8, 8, 0, 4, None, None) == -22
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a, a, a, 8, 8, 0, 2, None, None) == -22      # masked image without a mask
    assert b"mask" in lib.cid_last_error()
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a, a, a, 8, 8, 0, 1, a, None) == -22         # mask_latents without a mask
    assert lib.cid_tiny_encode_in_f16(a, 3, a, 2, a, a, a, 8, 8, 0, 3, None, None) == -22         # Bm = 2 beside Bi = 3
    assert b"Bm" in lib.cid_last_error()
    assert lib.cid_tiny_encode_in_f16(a, 1, a, 1, a, a, a, 8, 12, 0, 3, a, None) == -22           # mask_latents at 8 x 12
    assert b"multiples of 8" in lib.cid_last_error()
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a + 2, a, a, 8, 8, 0, 1, None, None) == -22
    assert lib.cid_tiny_encode_in_f16(a, 1, None, 0, a, a, a, 0, 8, 0, 1, None, None) == -22
    assert lib.cid_tiny_encode_out_f16(a, None, a, a, 1, 4, 4, 1.0, None) == -22
    assert lib.cid_tiny_encode_out_f16(a, a, a, a, 1, 4, -1, 1.0, None) == -22
    assert lib.cid_tiny_encode_out_f16(a + 2, a, a, a, 1, 4, 4, 1.0, None) == -22
    assert b"aligned" in lib.cid_last_error()


def test_ops_wrappers_refuse_before_any_launch(lib):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    x, out, w = h(1, 15, 64), h(1, 6, 64), h(64, 9, 64)              # 3 x 5 -> 2 x 3
    with pytest.raises(CidError, match=r"tiny_conv64_s2\.x: expected torch\.float16"):
        ops.tiny_conv64_s2(x.float(), out, w, B=1, H=3, W=5)
    with pytest.raises(CidError, match=r"tiny_conv64_s2\.x: expected shape"):
        ops.tiny_conv64_s2(h(1, 15, 32), out, w, B=1, H=3, W=5)
    with pytest.raises(CidError, match=r"tiny_conv64_s2\.out: expected shape"):
        ops.tiny_conv64_s2(x, h(1, 2, 64), w, B=1, H=3, W=5)        # floor(3 / 2) x floor(5 / 2): the sizes round UP
    with pytest.raises(CidError, match=r"tiny_conv64_s2\.w: expected shape"):
        ops.tiny_conv64_s2(x, out, h(64, 9, 32), B=1, H=3, W=5)
    with pytest.raises(CidError, match=r"tiny_conv64_s2\.x: tensor must be contiguous"):
        ops.tiny_conv64_s2(h(1, 64, 15).transpose(1, 2), out, w, B=1, H=3, W=5)
    with pytest.raises(CidError, match="must live on the GPU"):
        ops.tiny_conv64_s2(x, out, w, B=1, H=3, W=5)
    img, msk, o64, w_in, b = f(2, 3, 8, 16), f(2, 1, 8, 16), h(2, 128, 64), h(64, 9, 3), h(64)
    with pytest.raises(CidError, match=r"tiny_encode_in\.image: expected \[B, 3, H, W\]"):
        ops.tiny_encode_in(f(2, 4, 8, 16), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_encode_in\.image: expected torch\.float32"):
        ops.tiny_encode_in(img.half(), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_encode_in\.image: tensor must be contiguous"):
        ops.tiny_encode_in(f(2, 3, 16, 8).transpose(2, 3), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_encode_in\.blocks"):
        ops.tiny_encode_in(img, o64, w_in, b, blocks=0)
    with pytest.raises(CidError, match=r"tiny_encode_in\.out: expected shape"):
        ops.tiny_encode_in(img, o64, w_in, b, mask=msk, blocks=3)                # both blocks need [4, 128, 64]
    with pytest.raises(CidError, match=r"tiny_encode_in\.w: expected shape"):
        ops.tiny_encode_in(img, o64, h(64, 9, 4), b)
    with pytest.raises(CidError, match=r"tiny_encode_in\.mask: expected \[1 or 2, 1, 8, 16\]"):
        ops.tiny_encode_in(img, o64, w_in, b, mask=f(2, 1, 8, 8), blocks=2)
    with pytest.raises(CidError, match=r"tiny_encode_in\.mask: expected torch\.float32"):
        ops.tiny_encode_in(img, o64, w_in, b, mask=msk.half(), blocks=2)
    with pytest.raises(CidError, match=r"tiny_encode_in\.mask: the masked image and mask_latents need a mask"):
        ops.tiny_encode_in(img, o64, w_in, b, blocks=2)
    with pytest.raises(CidError, match=r"tiny_encode_in\.mask_latents: expected shape"):
        ops.tiny_encode_in(img, o64, w_in, b, mask=msk, mask_latents=h(2, 1, 2, 2))
    with pytest.raises(CidError, match=r"tiny_encode_in\.mask_latents: H and W must be multiples of 8"):
        ops.tiny_encode_in(f(2, 3, 8, 12), h(2, 96, 64), w_in, b, mask=f(2, 1, 8, 12), mask_latents=h(2, 1, 1, 1))
    with pytest.raises(CidError, match="must live on the GPU"):
        ops.tiny_encode_in(img, o64, w_in, b)
    lat, t64, w_out, b4 = h(2, 4, 3, 5), h(2, 15, 64), h(4, 9, 64), h(4)
    with pytest.raises(CidError, match=r"tiny_encode_out\.out: expected \[B, 4, H, W\]"):
        ops.tiny_encode_out(t64, h(2, 3, 3, 5), w_out, b4)
    with pytest.raises(CidError, match=r"tiny_encode_out\.x: expected shape"):
        ops.tiny_encode_out(h(2, 15, 32), lat, w_out, b4)
    with pytest.raises(CidError, match=r"tiny_encode_out\.x: expected torch\.float16"):
        ops.tiny_encode_out(t64.float(), lat, w_out, b4)
    with pytest.raises(CidError, match=r"tiny_encode_out\.w: expected shape"):
        ops.tiny_encode_out(t64, lat, h(3, 9, 64), b4)
    with pytest.raises(CidError, match=r"tiny_encode_out\.out: tensor must be contiguous"):
        ops.tiny_encode_out(t64, h(2, 4, 5, 3).transpose(2, 3), w_out, b4)
    with pytest.raises(CidError, match="must live on the GPU"):
        ops.tiny_encode_out(t64, lat, w_out, b4)


def test_reference_imports_only_its_sibling():
    import ast
    tree = ast.parse(open(E.__file__).read())
    names = [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + \
            [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert not any(n.split(".")[0] in ("consistentid_amd", "oracle") for n in names), names
    assert "taesd_ref" in names and E.AutoencoderTinyBlock is R.AutoencoderTinyBlock
