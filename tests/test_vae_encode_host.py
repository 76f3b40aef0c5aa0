"""VAE encoder, host side (no GPU): argument checks of the new entry points, the quant_conv fold, and the order of the
inpaint pipelines' random draws (diffusers 0.23 prepare_latents / prepare_mask_latents)."""
import ctypes as C

import pytest
import torch


def _desc(**kw):
    from consistentid_amd._lib import GemmDesc
    d = GemmDesc()
    d.x1, d.w, d.out = 64, 64, 64
    d.c1 = d.ld1 = d.ldo = d.N = 128
    d.taps, d.stride, d.pad_mode = 9, 2, 1
    d.Hi, d.Wi, d.Ho, d.Wo = 64, 64, 32, 32
    d.M = 2 * 32 * 32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pad_mode_argument_checks(lib):
    assert lib.cid_version() >= 101
    bad = [dict(stride=1, Ho=64, Wo=64, M=2 * 64 * 64),          # pad_mode 1 is a stride-2 rule
           dict(Hi=63, Ho=31, M=2 * 31 * 32),                      # odd Hi
           dict(Ho=31, M=2 * 31 * 32),                             # Ho != Hi / 2
           dict(Wo=31, M=2 * 32 * 31),                             # Wo != Wi / 2
           dict(up=1),
           dict(taps=1),
           dict(mode=1),
           dict(pad_mode=2)]
    for kw in bad:
        assert lib.cid_gemm_f16(C.byref(_desc(**kw)), None) == -22, kw
        assert b"pad_mode" in lib.cid_last_error(), (kw, lib.cid_last_error())
    assert lib.cid_gemm_f16(C.byref(_desc(x1=None)), None) == -22
    assert b"null pointer" in lib.cid_last_error()


def test_encode_in_argument_checks(lib):
    f = lib.cid_vae_encode_in_f16
    # (image, Bi, mask, Bm, out, w, bias, H, W, cout, normalize, blocks, mask_latents, stream)
    assert f(None, 1, None, 0, 64, 64, 64, 64, 64, 128, 1, 1, None, None) == -22
    assert b"null pointer" in lib.cid_last_error()
    assert f(64, 1, 64, 1, None, 64, 64, 64, 64, 128, 1, 3, None, None) == -22
    assert f(64, 2, 64, 3, 64, 64, 64, 64, 64, 128, 1, 3, None, None) == -22          # Bm not in {1, Bi}
    assert b"Bm=3" in lib.cid_last_error()
    assert f(64, 2, None, 0, 64, 64, 64, 64, 64, 128, 1, 3, None, None) == -22        # masked image without a mask
    assert b"need a mask" in lib.cid_last_error()
    assert f(64, 1, None, 0, 64, 64, 64, 64, 64, 128, 1, 1, 64, None) == -22          # mask latents without a mask
    assert f(64, 1, 64, 1, 64, 64, 64, 60, 64, 128, 1, 3, 64, None) == -22            # mask latents need H % 8 == 0
    assert b"multiples of 8" in lib.cid_last_error()
    assert f(64, 1, 64, 1, 64, 64, 64, 64, 64, 132, 1, 3, None, None) == -22          # cout % 8
    assert f(64, 1, 64, 1, 64, 64, 64, 64, 64, 128, 1, 0, None, None) == -22          # no block
    assert f(64, 1, 64, 1, 64, 64, 64, 64, 64, 128, 1, 4, None, None) == -22


def test_encode_out_argument_checks(lib):
    f = lib.cid_vae_encode_out_f16
    # (x, out, moments, w, bias, eps, B, H, W, cin, L, scale, stream)
    assert f(None, 64, None, 64, 64, None, 1, 64, 64, 512, 4, 0.18215, None) == -22
    assert b"null pointer" in lib.cid_last_error()
    assert f(64, 64, None, 64, None, None, 1, 64, 64, 512, 4, 0.18215, None) == -22    # bias
    assert f(64, 64, None, 64, 64, None, 1, 64, 64, 512, 5, 0.18215, None) == -22      # L <= 4
    assert f(64, 64, None, 64, 64, None, 1, 64, 64, 500, 4, 0.18215, None) == -22      # cin % 8
    assert f(64, 64, None, 64, 64, None, 0, 64, 64, 512, 4, 0.18215, None) == -22


def test_quant_conv_fold_matches_oracle():
    """W' = Q W per tap, b' = Q b + q_b (fp64) reproduces quant_conv(conv_out(x)) of the oracle modules."""
    from consistentid_amd import synth, vae_spec
    from consistentid_amd.vae import fold_quant_conv
    from oracle import vae as ovae
    cfg = vae_spec.tiny_vae_config()
    sd = synth.random_vae_state_dict(cfg, seed=5)
    oracle = ovae.AutoencoderKL(ovae.tiny_vae_config()).double().eval()
    oracle.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    w, b = fold_quant_conv(sd["encoder.conv_out.weight"].double(), sd["encoder.conv_out.bias"].double(),
                           sd["quant_conv.weight"].double(), sd["quant_conv.bias"].double())
    x = torch.randn(2, cfg.block_out_channels[-1], 9, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        ref = oracle.quant_conv(oracle.encoder.conv_out(x))
        got = torch.nn.functional.conv2d(x, w, b, padding=1)
    assert w.shape == (2 * cfg.latent_channels, cfg.block_out_channels[-1], 3, 3)
    assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max()) * 100


@pytest.mark.parametrize("unet_channels", [4, 9])
@pytest.mark.parametrize("strength", [1.0, 0.6])
@pytest.mark.parametrize("latents_given", [False, True])
def test_inpaint_draw_order(unet_channels, strength, latents_given):
    """pipeline.inpaint_draws consumes a generator exactly like diffusers 0.23's inpaint pipelines: eps of the init image
    (4-channel UNet, or no latents with strength < 1), noise (no latents), eps of the masked image (always)."""
    from consistentid_amd.pipeline import inpaint_draws
    Bi, B, L, h, w = 1, 2, 4, 6, 5
    g = torch.Generator().manual_seed(1234)
    eps_i, noise, eps_m = inpaint_draws(g, image_batch=Bi, batch_size=B, latent_channels=L, h=h, w=w,
                                        unet_channels=unet_channels, latents_given=latents_given, strength=strength,
                                        device="cpu")
    r = torch.Generator().manual_seed(1234)
    draw = lambda *shape: torch.randn(shape, generator=r, dtype=torch.float16)
    want_i = draw(Bi, L, h, w) if (unet_channels == 4 or (not latents_given and strength < 1.0)) else None
    want_n = draw(B, L, h, w) if not latents_given else None
    want_m = draw(Bi, L, h, w)
    for got, want in ((eps_i, want_i), (noise, want_n), (eps_m, want_m)):
        assert (got is None) == (want is None)
        if want is not None:
            assert got.dtype == torch.float16 and torch.equal(got, want)
    assert torch.equal(g.get_state(), r.get_state())          # nothing else was drawn


def test_randn_tensor_rules():
    from consistentid_amd.vae import randn_tensor
    g = torch.Generator().manual_seed(3)
    a = randn_tensor((2, 3), generator=g, device="cpu")
    assert a.dtype == torch.float16 and torch.equal(a, torch.randn((2, 3), generator=torch.Generator().manual_seed(3),
                                                                   dtype=torch.float16))
    with pytest.raises(NotImplementedError):
        randn_tensor((2, 3), generator=[g, g], device="cpu")
