"""AutoencoderTiny (TAESD) on the host: weight packing, the config / state-dict refusals, the loader's dispatch on
``_class_name``, the ABI and the argument checks of the ops wrappers.  No GPU: the engine is never built here (its constructor
moves the packed weights to the device); everything it decides on the host is a pure function of vae_tiny."""
import json
import os

import pytest
import torch

import taesd_ref as R


@pytest.fixture(scope="module")
def model():
    return R.synthetic(3)


@pytest.fixture(scope="module")
def sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ----------------------------------------------------------------------------- packing
def test_layer_walk_of_the_published_decoder():
    from consistentid_amd.vae_tiny import tiny_decoder_layers
    walk = tiny_decoder_layers((3, 3, 3, 1))
    assert walk == [("in", 0), ("block", 2), ("block", 3), ("block", 4), ("upconv", 6), ("block", 7), ("block", 8), ("block", 9),
                    ("upconv", 11), ("block", 12), ("block", 13), ("block", 14), ("upconv", 16), ("block", 17), ("out", 18)]
    assert tiny_decoder_layers((1, 2)) == [("in", 0), ("block", 2), ("upconv", 4), ("block", 5), ("block", 6), ("out", 7)]


def test_packing_maps_diffusers_keys(model, sd):
    from consistentid_amd.vae_tiny import pack_tiny_decoder
    walk, packed = pack_tiny_decoder(R.config(), sd)
    assert walk[-1] == ("out", 18)
    # every tensor: fp16, contiguous, the kernels' [N][9][C]
    for k, t in packed.items():
        assert t.dtype == torch.float16 and t.is_contiguous(), k
    assert packed["0.w"].shape == (64, 9, 4) and packed["0.b"].shape == (64,)
    assert packed["18.w"].shape == (3, 9, 64) and packed["18.b"].shape == (3,)
    for i in (2, 3, 4, 7, 8, 9, 12, 13, 14, 17):
        for j in (0, 2, 4):
            assert packed[f"{i}.{j}.w"].shape == (64, 9, 64) and packed[f"{i}.{j}.b"].shape == (64,)
            assert torch.equal(packed[f"{i}.{j}.b"].float(), sd[f"decoder.layers.{i}.conv.{j}.bias"])
    # the convs after an Upsample carry no bias
    for i in (6, 11, 16):
        assert packed[f"{i}.w"].shape == (64, 9, 64) and f"{i}.b" not in packed
        assert f"decoder.layers.{i}.bias" not in sd
    assert torch.equal(packed["0.b"].float(), sd["decoder.layers.0.bias"])
    assert torch.equal(packed["18.b"].float(), sd["decoder.layers.18.bias"])
    # nothing else: 2 + 10 * 6 + 3 + 2 tensors
    assert len(packed) == 67
    # one tap of one layer against the torch weight: tap = 3 ky + kx, [cout][tap][cin]
    w = sd["decoder.layers.8.conv.2.weight"]               # [64, 64, 3, 3]
    ky, kx = 2, 0
    assert torch.equal(packed["8.2.w"][:, 3 * ky + kx, :].float(), w[:, :, ky, kx])
    assert float(packed["8.2.w"][5, 7, 11]) == float(w[5, 11, 2, 1])
    assert torch.equal(packed["0.w"][:, 1, :].float(), sd["decoder.layers.0.weight"][:, :, 0, 1])
    assert torch.equal(packed["16.w"][:, 5, :].float(), sd["decoder.layers.16.weight"][:, :, 1, 2])


def test_packing_ignores_the_encoder_and_takes_other_block_counts(sd):
    from consistentid_amd.vae_tiny import pack_tiny_decoder
    with_enc = dict(sd)
    with_enc["encoder.layers.0.weight"] = torch.zeros(64, 3, 3, 3)
    assert set(pack_tiny_decoder(R.config(), with_enc)[1]) == set(pack_tiny_decoder(R.config(), sd)[1])
    small = R.synthetic(1, (1, 2))
    walk, packed = pack_tiny_decoder(R.config((1, 2)), small.state_dict())
    assert walk[-1] == ("out", 7) and "4.w" in packed and "4.b" not in packed and packed["7.w"].shape == (3, 9, 64)


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("key,value", [("act_fn", "swish"), ("decoder_block_out_channels", [64, 64, 128, 64]),
                                       ("block_out_channels", [64, 32, 64, 64]), ("latent_channels", 16), ("out_channels", 4),
                                       ("upsampling_scaling_factor", 4), ("num_decoder_blocks", [3, 0, 3, 1]),
                                       ("num_decoder_blocks", [])])
def test_config_refusals_name_the_key(sd, key, value):
    from consistentid_amd.vae_tiny import HipAutoencoderTiny

    class Untouchable(dict):
        """a state dict that must not be read: the config is refused before any weight is touched"""
        def __getitem__(self, k):
            raise AssertionError(f"weight {k} was read before the config was checked")

        def __iter__(self):
            raise AssertionError("the state dict was walked before the config was checked")

    cfg = R.config()
    cfg[key] = value
    with pytest.raises(NotImplementedError, match=key):
        HipAutoencoderTiny(cfg, Untouchable(), device="cpu")


def test_layer_list_that_does_not_match_num_decoder_blocks(sd):
    from consistentid_amd.vae_tiny import pack_tiny_decoder
    with pytest.raises(NotImplementedError, match="num_decoder_blocks"):
        pack_tiny_decoder(R.config((3, 3, 3, 2)), sd)              # one Block more than the weights have
    with pytest.raises(NotImplementedError, match="num_decoder_blocks"):
        pack_tiny_decoder(R.config((3, 3, 1)), sd)


def test_missing_and_unexpected_decoder_keys(sd):
    from consistentid_amd.vae_tiny import pack_tiny_decoder
    gone = {k: v for k, v in sd.items() if k != "decoder.layers.9.conv.2.bias"}
    with pytest.raises(NotImplementedError, match=r"decoder\.layers\.9\.conv\.2\.bias"):
        pack_tiny_decoder(R.config(), gone)
    extra = dict(sd)
    extra["decoder.layers.6.bias"] = torch.zeros(64)                # the conv after an Upsample has no bias
    with pytest.raises(NotImplementedError, match=r"decoder\.layers\.6\.bias"):
        pack_tiny_decoder(R.config(), extra)
    skip = dict(sd)
    skip["decoder.layers.3.skip.weight"] = torch.zeros(64, 64, 1, 1)
    with pytest.raises(NotImplementedError, match=r"decoder\.layers\.3\.skip\.weight"):
        pack_tiny_decoder(R.config(), skip)
    shape = dict(sd)
    shape["decoder.layers.0.weight"] = torch.zeros(64, 8, 3, 3)
    with pytest.raises(NotImplementedError, match=r"decoder\.layers\.0\.weight"):
        pack_tiny_decoder(R.config(), shape)


def test_encode_is_not_built():
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    with pytest.raises(NotImplementedError, match="AutoencoderTiny.encode is not built"):
        HipAutoencoderTiny.encode(object.__new__(HipAutoencoderTiny), torch.zeros(1, 3, 8, 8))


def test_exported_from_the_package():
    import consistentid_amd
    from consistentid_amd.vae_tiny import HipAutoencoderTiny
    assert consistentid_amd.HipAutoencoderTiny is HipAutoencoderTiny and "HipAutoencoderTiny" in consistentid_amd.__all__


# ----------------------------------------------------------------------------- loader
class _Built:
    """stands in for an engine class: records what the loader hands it (no GPU here)"""
    def __init__(self, *a, **kw):
        self.args, self.kw = a, kw


def test_loader_dispatches_on_class_name(tmp_path, model, monkeypatch):
    from consistentid_amd import loader, synth, vae, vae_spec, vae_tiny
    tiny = type("Tiny", (_Built,), {})
    kl = type("KL", (_Built,), {})
    monkeypatch.setattr(vae_tiny, "HipAutoencoderTiny", tiny)
    monkeypatch.setattr(vae, "make_vae_decoder", lambda cfg, sd, device="cuda:0": kl(cfg, sd, device=device))
    # a stand-alone taesd folder, and the same folder as <root>/vae
    R.write_folder(tmp_path / "taesd", model)
    R.write_folder(tmp_path / "root" / "vae", model)
    got = loader.load_tiny_vae(tmp_path / "taesd", device="cpu")
    assert type(got) is tiny and got.args[0]["_class_name"] == "AutoencoderTiny" and got.kw == {"device": "cpu"}
    assert set(got.args[1]) == set(model.state_dict()) and got.args[1]["decoder.layers.18.bias"].dtype == torch.float16
    assert type(loader.load_vae(tmp_path / "root", device="cpu")) is tiny
    # a KL config still builds what it built: VAEConfig through make_vae_decoder
    vcfg = vae_spec.tiny_vae_config()
    from safetensors.torch import save_file
    os.makedirs(tmp_path / "kl" / "vae")
    kl_cfg = {"_class_name": "AutoencoderKL", "in_channels": vcfg.in_channels, "out_channels": vcfg.out_channels,
              "latent_channels": vcfg.latent_channels, "block_out_channels": list(vcfg.block_out_channels),
              "layers_per_block": vcfg.layers_per_block, "norm_num_groups": vcfg.norm_num_groups,
              "scaling_factor": vcfg.scaling_factor, "force_upcast": vcfg.force_upcast}
    with open(tmp_path / "kl" / "vae" / "config.json", "w") as f:
        json.dump(kl_cfg, f)
    save_file({k: v.cpu().contiguous() for k, v in synth.random_vae_state_dict(vcfg, seed=5, device="cpu").items()},
              str(tmp_path / "kl" / "vae" / "diffusion_pytorch_model.safetensors"))
    got = loader.load_vae(tmp_path / "kl", device="cpu")
    assert type(got) is kl and got.args[0] == loader.vae_config_from_diffusers(kl_cfg)
    no_name = dict(kl_cfg)
    del no_name["_class_name"]
    assert not loader.is_tiny_vae(no_name) and not loader.is_tiny_vae(kl_cfg) and loader.is_tiny_vae(R.config())
    # load_tiny_vae refuses a KL folder by name
    with pytest.raises(NotImplementedError, match="AutoencoderKL"):
        loader.load_tiny_vae(tmp_path / "kl" / "vae", device="cpu")


def test_from_pretrained_takes_a_built_vae(tmp_path, monkeypatch):
    """``vae=`` replaces the folder's decoder; without the keyword the folder's decoder is built as before; junk is refused
    before anything is read"""
    from consistentid_amd import loader, pipeline
    with pytest.raises(TypeError, match="vae="):
        loader.from_pretrained(pipeline.ConsistentIDStableDiffusionPipeline, tmp_path / "nowhere", vae="madebyollin/taesd")
    seen = {}

    class Pipe(pipeline.ConsistentIDStableDiffusionPipeline):
        def __init__(self, unet, **kw):
            seen.update(kw)

    monkeypatch.setattr(loader, "load_unet", lambda root, device="cuda:0": "unet")
    monkeypatch.setattr(loader, "_make_decoder", lambda cfg, sd, device: ("folder decoder", cfg["_class_name"]))
    R.write_folder(tmp_path / "base" / "vae", R.synthetic(0))
    mine = _Built()
    mine.decode_latents = lambda x: x
    loader.from_pretrained(Pipe, tmp_path / "base", vae=mine)
    assert seen["vae"] is mine
    seen.clear()
    loader.from_pretrained(Pipe, tmp_path / "base")
    assert seen["vae"] == ("folder decoder", "AutoencoderTiny") and "vae_encoder" not in seen


# ----------------------------------------------------------------------------- ABI and wrappers
def test_abi_exports_and_version(lib):
    for name in ("cid_tiny_conv64_f16", "cid_tiny_decode_in_f16", "cid_tiny_decode_out_f16", "cid_tiny_conv64_tile"):
        assert hasattr(lib, name), name
    assert lib.cid_version() >= 112
    from consistentid_amd import ops
    th, tw, cap = ops.tiny_conv64_tile()
    assert th >= 1 and tw >= 1 and cap >= 1


def test_c_entries_refuse_bad_arguments_before_any_launch(lib):
    """-22 with a text, on a machine without a GPU: nothing is launched for a refused call"""
    a = 4096                                  # an aligned stand-in address: refused calls never dereference it
    assert lib.cid_tiny_conv64_f16(None, a, a, None, None, 1, 4, 4, 0, 0, None) == -22
    assert b"null" in lib.cid_last_error()
    assert lib.cid_tiny_conv64_f16(a, 2 * a, a, None, None, 1, 0, 4, 0, 0, None) == -22
    assert lib.cid_tiny_conv64_f16(a, 2 * a, a, None, None, 1, 4, 4, 2, 0, None) == -22
    assert b"up" in lib.cid_last_error()
    assert lib.cid_tiny_conv64_f16(a, 2 * a, a, None, None, 1, 4, 4, 0, 3, None) == -22
    assert lib.cid_tiny_conv64_f16(a, 2 * a + 8, a, None, None, 1, 4, 4, 0, 0, None) == -22
    assert b"aligned" in lib.cid_last_error()
    assert lib.cid_tiny_conv64_f16(a, a, a + 64, None, None, 1, 4, 4, 0, 0, None) == -22
    assert b"alias" in lib.cid_last_error()
    assert lib.cid_tiny_decode_in_f16(a, None, a, a, 1, 4, 4, None) == -22
    assert lib.cid_tiny_decode_in_f16(a, a, a, a, 1, 4, -1, None) == -22
    assert lib.cid_tiny_decode_out_f16(a, a, a, a, 1, 4, 4, 2, None) == -22
    assert b"mode" in lib.cid_last_error()
    assert lib.cid_tiny_decode_out_f16(a + 2, a, a, a, 1, 4, 4, 0, None) == -22


def test_ops_wrappers_refuse_before_any_launch(lib):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    x, out, w, b = h(1, 16, 64), h(1, 16, 64), h(64, 9, 64), h(64)
    with pytest.raises(CidError, match=r"tiny_conv64\.x: expected torch\.float16"):
        ops.tiny_conv64(x.float(), out, w, b, B=1, H=4, W=4)
    with pytest.raises(CidError, match=r"tiny_conv64\.w: expected torch\.float16"):
        ops.tiny_conv64(x, out, w.float(), b, B=1, H=4, W=4)
    with pytest.raises(CidError, match=r"tiny_conv64\.x: expected shape"):
        ops.tiny_conv64(h(1, 16, 32), out, w, b, B=1, H=4, W=4)                 # 32 channels
    with pytest.raises(CidError, match=r"tiny_conv64\.w: expected shape"):
        ops.tiny_conv64(x, out, h(64, 9, 32), b, B=1, H=4, W=4)
    with pytest.raises(CidError, match=r"tiny_conv64\.out: expected shape"):
        ops.tiny_conv64(x, out, w, b, B=1, H=4, W=4, up=True)                   # up needs [1, 64, 64]
    with pytest.raises(CidError, match=r"tiny_conv64\.res: expected shape"):
        ops.tiny_conv64(x, out, w, b, B=1, H=4, W=4, res=h(1, 8, 64))
    with pytest.raises(CidError, match=r"tiny_conv64\.x: tensor must be contiguous"):
        ops.tiny_conv64(h(1, 64, 16).transpose(1, 2), out, w, b, B=1, H=4, W=4)
    z, o64, w_in = h(2, 4, 3, 5), h(2, 15, 64), h(64, 9, 4)
    with pytest.raises(CidError, match=r"tiny_decode_in\.z: expected \[B, 4, h, w\]"):
        ops.tiny_decode_in(h(2, 8, 3, 5), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_decode_in\.z: expected torch\.float16"):
        ops.tiny_decode_in(z.float(), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_decode_in\.z: tensor must be contiguous"):
        ops.tiny_decode_in(h(2, 4, 5, 3).transpose(2, 3), o64, w_in, b)
    with pytest.raises(CidError, match=r"tiny_decode_in\.w: expected shape"):
        ops.tiny_decode_in(z, o64, h(64, 9, 8), b)
    img, w_out, b3 = h(2, 3, 3, 5), h(3, 9, 64), h(3)
    with pytest.raises(CidError, match=r"tiny_decode_out\.out: expected \[B, 3, H, W\]"):
        ops.tiny_decode_out(o64, h(2, 4, 3, 5), w_out, b3)
    with pytest.raises(CidError, match=r"tiny_decode_out\.x: expected shape"):
        ops.tiny_decode_out(h(2, 15, 32), img, w_out, b3)
    with pytest.raises(CidError, match=r"tiny_decode_out\.x: expected torch\.float16"):
        ops.tiny_decode_out(o64.float(), img, w_out, b3)
    with pytest.raises(CidError, match=r"tiny_decode_out\.out: tensor must be contiguous"):
        ops.tiny_decode_out(o64, h(2, 3, 5, 3).transpose(2, 3), w_out, b3)
    # well-formed operands on the CPU: refused for the device, still before any launch
    with pytest.raises(CidError, match="must live on the GPU"):
        ops.tiny_conv64(x, out, w, b, B=1, H=4, W=4)


def test_reference_does_not_import_the_product():
    import ast
    tree = ast.parse(open(R.__file__).read())
    names = [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)] + \
            [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert not any(n.split(".")[0] in ("consistentid_amd", "oracle") for n in names), names
