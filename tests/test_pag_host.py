"""Host side of perturbed-attention guidance: the layer ids, the folded to_out . to_v weights against
a float64 composition, the embed-row selectors and the per-step scale column, every refusal the pipelines and the engine
make before a launch, and the argument checks of the three step entries.  No GPU."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from consistentid_amd import scheduler as S
from consistentid_amd import unet_spec as U

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("cid_cfg_pag_ddim_step_f16", "cid_cfg_pag_multistep_step_f16", "cid_pag_multistep_step_f16")


def _same_bits(a, b):
    """(the fold vectors are fp32 bits in fp16-typed tensors: some halves read as NaN, which torch.equal never finds equal)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _all_blocks(cfg):
    downs, mid, ups = U.walk(cfg)
    return [f"{t.name}.transformer_blocks.{k}" for blk in downs + [mid] + ups for t in blk.attentions for k in range(t.n_layers)]


# ----------------------------------------------------------------------------------------------------------- layer ids
@pytest.mark.parametrize("cfg", [U.tiny_config("sd15"), U.tiny_config("sdxl"), U.sd15_config(), U.sdxl_config()],
                         ids=["tiny", "tinyxl", "sd15", "sdxl"])
def test_mid_is_the_mid_blocks_self_attentions_and_the_default(cfg):
    want = [b for b in _all_blocks(cfg) if b.startswith("mid_block.")]
    assert len(want) == cfg.transformer_layers_per_block[-1] >= 1
    assert U.pag_blocks(cfg, "mid") == U.pag_blocks(cfg, ["mid"]) == U.pag_blocks(cfg) == want
    assert U.pag_blocks(cfg, "mid_block") == U.pag_blocks(cfg, "mid_block.attentions.0") == want
    assert U.PAG_DEFAULT_LAYERS == ("mid",)


def test_ids_select_whole_modules_in_execution_order():
    cfg = U.sd15_config()
    blocks = _all_blocks(cfg)
    assert len(blocks) == 16
    d1 = [b for b in blocks if b.startswith("down_blocks.1.")]
    assert U.pag_blocks(cfg, "down.block_1") == U.pag_blocks(cfg, "down_blocks.1") == d1 and len(d1) == 2
    assert U.pag_blocks(cfg, "down.block_1.attentions_1") == U.pag_blocks(cfg, "down_blocks.1.attentions.1") == [d1[1]]
    assert U.pag_blocks(cfg, "up.block_3.attentions_2") == ["up_blocks.3.attentions.2.transformer_blocks.0"]
    assert U.pag_blocks(cfg, "up_blocks.3.attentions.2.transformer_blocks.0.attn1") == ["up_blocks.3.attentions.2.transformer_blocks.0"]
    # given out of order and twice: execution order (down, mid, up), once each
    got = U.pag_blocks(cfg, ["up.block_1", "mid", "down.block_0", "mid", "down.block_0.attentions_0"])
    assert got == [b for b in blocks if b.startswith(("down_blocks.0.", "mid_block.", "up_blocks.1."))] and len(got) == 2 + 1 + 3
    assert U.pag_blocks(cfg, ["down.block_0", "down.block_1", "down.block_2", "mid", "up.block_1", "up.block_2", "up.block_3"]) == blocks
    xl = U.sdxl_config()
    assert len(U.pag_blocks(xl, "mid")) == 10 and len(U.pag_blocks(xl, "down.block_2.attentions_1")) == 10
    assert len(U.pag_blocks(xl, "up.block_1")) == 6 and len(U.pag_blocks(xl, "down.block_1")) == 4


def test_components_match_whole_never_by_prefix():
    """a UNet with eleven down blocks: ``down.block_1`` is block 1 alone, never block 10"""
    n = 11
    cfg = U.UNetConfig(block_out_channels=(64,) * n, down_block_types=("CrossAttnDownBlock2D",) * n,
                       up_block_types=("CrossAttnUpBlock2D",) * n, layers_per_block=1, transformer_layers_per_block=(1,) * n,
                       num_attention_heads=(2,) * n)
    assert U.pag_blocks(cfg, "down.block_1") == ["down_blocks.1.attentions.0.transformer_blocks.0"]
    assert U.pag_blocks(cfg, "down_blocks.1") == ["down_blocks.1.attentions.0.transformer_blocks.0"]
    assert U.pag_blocks(cfg, "down.block_10") == ["down_blocks.10.attentions.0.transformer_blocks.0"]
    assert U.pag_blocks(cfg, "up.block_1.attentions_1") == ["up_blocks.1.attentions.1.transformer_blocks.0"]
    with pytest.raises(ValueError, match="down_blocks.1.attentions.0.transformer_blocks.0.attn"):
        U.pag_blocks(cfg, "down_blocks.1.attentions.0.transformer_blocks.0.attn")     # "attn" is no component of "attn1"


@pytest.mark.parametrize("bad", ["", "middle", "down.block_7", "down.block_3", "up.block_0", "mid.attentions_1", "down", "block_1",
                                 "mid_block.attentions.0.transformer_blocks.0.attn2", "down.block_1.attentions_2"])
def test_an_id_that_selects_nothing_is_named(bad):
    """SD1.5: down block 3 and up block 0 have no attention; attn2 is cross-attention"""
    with pytest.raises(ValueError, match=re.escape(repr(bad))):
        U.pag_blocks(U.sd15_config(), ["mid", bad])
    for layers in ([], (), None, 3, ["mid", 3]):
        with pytest.raises(ValueError, match="pag_applied_layers"):
            U.pag_blocks(U.sd15_config(), layers)


# ----------------------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("c,seed", [(64, 0), (128, 1), (320, 2)])
def test_fold_vo_against_float64(c, seed):
    """W' = (Wo Wv) diag(gamma) rounded ONCE to fp16: every element within half an fp16 ulp (2^-11 relative; 2^-25 absolute
    below the normal range) of the float64 composition plus the fp32 product's own error, bounded by c * 2^-23 * |Wo| |Wv|.  s is
    the row sum of the ROUNDED W' (so that the mean term cancels on a constant row), b' = Wvo beta + bias, both fp32: held to
    c * 2^-22 of the sum of magnitudes.  And the folded map applied to a LayerNorm-ed row in float64 reproduces
    to_out(to_v(LN(x))) to fp16 weight precision."""
    from consistentid_amd.weights import fold_ln, fold_vo
    g = torch.Generator().manual_seed(seed)
    wv, wo = (torch.randn(c, c, generator=g) / c ** 0.5 for _ in range(2))
    gamma, beta, bias = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wl, s, b = fold_vo(wv, wo, gamma, beta, bias)
    assert wl.dtype == s.dtype == b.dtype == torch.float16 and tuple(wl.shape) == (c, c) and wl.is_contiguous()
    s, b = s.view(torch.float32), b.view(torch.float32)
    assert tuple(s.shape) == tuple(b.shape) == (c,)
    wvo = wo.double() @ wv.double()
    want = wvo * gamma.double()[None]
    slack = c * 2.0 ** -23 * (wo.double().abs() @ wv.double().abs()) * gamma.double().abs()[None]
    assert ((wl.double() - want).abs() <= want.abs() * 2.0 ** -11 + 2.0 ** -25 + slack).all()
    assert torch.equal(s, wl.float().sum(1)) or (s.double() - wl.double().sum(1)).abs().max() <= c * 2.0 ** -22 * wl.double().abs().sum(1).max()
    want_b = wvo @ beta.double() + bias.double()
    assert (b.double() - want_b).abs().max() <= c * 2.0 ** -22 * ((wvo.abs() @ beta.double().abs()) + bias.double().abs()).max()
    # without a bias b' is W beta alone, and the triple is fold_ln's of the fp32 product
    wl0, s0, b0 = fold_vo(wv, wo, gamma, beta)
    ref = fold_ln(wo @ wv, gamma, beta)
    assert all(_same_bits(a, r) for a, r in zip((wl0, s0, b0), ref)) and _same_bits(wl0, wl)
    # the whole map on rows: rstd * (x W'^T - mean * s) + b'  ==  to_out(to_v(LN(x))) + bias
    x = torch.randn(5, c, generator=g).double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    got = rstd * (x @ wl.double().T - mean * s.double()[None]) + b.double()[None]
    ln = (x - mean) * rstd * gamma.double()[None] + beta.double()[None]
    full = ln @ wv.double().T @ wo.double().T + bias.double()[None]
    assert float((got - full).norm() / full.norm()) <= 2.0 ** -10


def test_packed_unet_keeps_pag_weights_beside_the_packed_set():
    """on the CPU (the packing is torch): the folded tensors live in ``pag``, never in ``w``; a block that stays selected keeps its
    tensors; without keep_base the RuntimeError names it"""
    from consistentid_amd import synth
    from consistentid_amd.weights import PAG_SUFFIXES, PackedUNet
    cfg = U.tiny_config("sd15")
    sd = synth.random_unet_state_dict(cfg, seed=0)
    ad = synth.random_adapter_state_dict(cfg, sd, rank=8, seed=1)
    plain = PackedUNet(cfg, sd, ad, "cpu")
    with pytest.raises(RuntimeError, match="keep_base=True"):
        plain.set_pag(U.pag_blocks(cfg, "mid"))
    assert plain.pag == {} and plain.set_pag(()).pag == {}
    p = PackedUNet(cfg, sd, ad, "cpu", keep_base=True)
    keys, nbytes = set(p.w), p.nbytes()
    assert keys == set(plain.w) and nbytes == plain.nbytes()
    mid = U.pag_blocks(cfg, "mid")
    p.set_pag(mid)
    assert set(p.w) == keys and p.nbytes() == nbytes and not any(".vo." in k for k in p.w)
    assert set(p.pag) == {f"{mid[0]}.attn1.vo.{x}" for x in PAG_SUFFIXES}
    held = {k: (v, v.clone()) for k, v in p.pag.items()}
    p.set_pag(mid + U.pag_blocks(cfg, "down.block_0"))
    assert len(p.pag) == 8 and all(p.pag[k] is v for k, (v, _) in held.items())
    # the same operands the engine merges: Wo' Wv' of the adapter-merged fp32 weights
    b = mid[0]
    idx = U.attn_processor_names(cfg).index(f"{b}.attn1.processor")
    mrg = lambda which, key: sd[f"{b}.attn1.{key}.weight"].half().double() + (
        ad[f"{idx}.to_{which}_lora.up.weight"].double() @ ad[f"{idx}.to_{which}_lora.down.weight"].double())
    wvo = mrg("out", "to_out.0") @ mrg("v", "to_v")
    w = p.pag[f"{b}.attn1.vo.w"]
    assert float((w.double() - wvo).norm() / wvo.norm()) <= 2.0 ** -11
    wl = p.pag[f"{b}.attn1.vo.wl"].double()
    gamma = sd[f"{b}.norm1.weight"].half().double()
    assert float((wl - wvo * gamma[None]).norm() / (wvo * gamma[None]).norm()) <= 2.0 ** -11
    # a repack (what load_adapter_modules and set_lora run) rewrites them in place, to the same bits from the same operands
    p._repack_attention(with_ip=False)
    assert all(p.pag[k] is v and _same_bits(v, old) for k, (v, old) in held.items())
    p.set_pag(())
    assert p.pag == {} and set(p.w) == keys and p.nbytes() == nbytes


# ----------------------------------------------------------------------------------------------------------- rows and scales
@pytest.mark.parametrize("null_post", [False, True])
def test_step_rows_gain_the_perturbed_columns(null_post):
    from consistentid_amd.denoise import step_rows
    B, n_ts = 3, 5
    for first, merge in ((0, 1), (2, 0), (0, 9)):
        base = step_rows(n_ts, first, merge, B, null_post)
        pag = step_rows(n_ts, first, merge, B, null_post, pag=True)
        assert tuple(pag.unet.shape) == (n_ts, 3 * B) and pag.unet.dtype == torch.int32
        assert torch.equal(pag.unet[:, :2 * B], base.unet), "the first 2B columns are the rows without PAG"
        assert torch.equal(pag.unet[:, 2 * B:], base.unet[:, B:]), "the perturbed rows read the conditional rows' context"
        assert torch.equal(pag.merged, base.merged) and torch.equal(pag.controlnet, base.controlnet)
        one = step_rows(n_ts, first, merge, B, null_post, single_pass=True)
        both = step_rows(n_ts, first, merge, B, null_post, single_pass=True, pag=True)
        assert tuple(both.unet.shape) == (n_ts, 2 * B)
        assert torch.equal(both.unet[:, :B], one.unet) and torch.equal(both.unet[:, B:], one.unet)
        for i in range(n_ts):       # text-only [B, 2B) up to the merge, augmented [2B, 3B) after it
            want = [b + (2 * B if (i - first) > merge else B) for b in range(B)]
            assert pag.unet[i, 2 * B:].tolist() == want == both.unet[i, B:].tolist()


def test_scale_column():
    from consistentid_amd.denoise import check_pag, pag_scale_column
    sch = S.DDIMScheduler()
    sch.set_timesteps(4)
    ts = sch.timesteps
    col = pag_scale_column(3.0, 0.0, ts)
    assert col.dtype == np.float32 and col.tolist() == [3.0] * 4
    col = pag_scale_column(3.0, 0.005, ts)          # timesteps 751, 501, 251, 1: 1.755, 0.505, then negative -> 0
    want = [max(3.0 - 0.005 * (1000 - int(t)), 0.0) for t in ts]
    assert np.allclose(col, want, rtol=0, atol=1e-6) and col[0] > col[1] > 0.0
    assert col[-1] == 0.0 and want[-1] == 0.0, "the clamp: a late timestep would give a negative scale"
    assert (col >= 0.0).all()
    lcm = S.LCMScheduler()
    lcm.set_timesteps(4)
    col = pag_scale_column(2.0, 0.004, lcm.timesteps)       # timesteps 999, 759, 519, 279: 1.996, 1.036, 0.076, then -0.884 -> 0
    assert np.allclose(col[:3], [1.996, 1.036, 0.076], rtol=0, atol=1e-6) and col[3] == 0.0
    assert check_pag(3, 0) == (3.0, 0.0) and check_pag(np.float32(0.5), 0.25) == (0.5, 0.25)
    for bad in (-1.0, float("nan"), float("inf"), True, "3", None):
        with pytest.raises(ValueError, match="pag_scale"):
            check_pag(bad, 0.0)
        with pytest.raises(ValueError, match="pag_adaptive_scale"):
            check_pag(1.0, bad)


# ----------------------------------------------------------------------------------------------------------- refusals
class _StubUNet(SimpleNamespace):
    """what the pipelines and the engine touch of a UNet before the first launch"""

    def __init__(self):
        super().__init__(device="cpu", config=U.tiny_config("sd15"), pag_layers=(), enabled=[])

    def enable_pag(self, layers=U.PAG_DEFAULT_LAYERS):
        self.enabled.append(layers)
        self.pag_layers = tuple(U.pag_blocks(self.config, layers))

    def disable_pag(self):
        self.pag_layers = ()


def _pipes():
    from consistentid_amd import pipeline
    return {"sd15": pipeline.ConsistentIDStableDiffusionPipeline, "sdxl": pipeline.ConsistentIDStableDiffusionXLPipeline,
            "inpaint": pipeline.StableDiffusionInpaintConsistentIDPipeline,
            "controlnet": pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline}


def test_call_signatures_and_enable_disable():
    import inspect
    for name, cls in _pipes().items():
        sig = inspect.signature(cls.__call__).parameters
        assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0, name
        pipe = cls(_StubUNet(), use_graph=False)
        pipe.enable_pag()
        assert pipe.unet.enabled == ["mid"] and pipe.unet.pag_layers == ("mid_block.attentions.0.transformer_blocks.0",)
        pipe.enable_pag(pag_applied_layers=["down.block_1", "mid"])
        assert len(pipe.unet.pag_layers) == 2
        with pytest.raises(ValueError, match="'down.block_9'"):
            pipe.enable_pag("down.block_9")
        pipe.disable_pag()
        assert pipe.unet.pag_layers == ()
    from consistentid_amd.denoise import DenoiseEngine
    sig = inspect.signature(DenoiseEngine.run).parameters
    assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0
    from consistentid_amd.unet import HipUNet
    assert inspect.signature(HipUNet.forward_tokens).parameters["pag_rows"].default == 0
    assert callable(HipUNet.enable_pag) and callable(HipUNet.disable_pag)


@pytest.mark.parametrize("name", ["sd15", "sdxl", "inpaint", "controlnet"])
def test_pipelines_validate_and_refuse_before_anything_runs(name):
    """the values like enable_freeu's (finite, not negative: ValueError); PAG with guidance_rescale and PAG on the ControlNet
    pipeline: NotImplementedError -- all before the pre-loop, so the stub UNet and missing inputs are never reached"""
    pipe = _pipes()[name](_StubUNet(), use_graph=False)
    for bad in (-0.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="pag_scale"):
            pipe(pag_scale=bad)
        with pytest.raises(ValueError, match="pag_adaptive_scale"):
            pipe(pag_scale=3.0, pag_adaptive_scale=bad)
    with pytest.raises(NotImplementedError, match="PAG with ControlNet residuals" if name == "controlnet" else "guidance_rescale"):
        pipe(pag_scale=3.0, guidance_rescale=0.7)
    assert pipe.unet.enabled == [], "a refused call must not change the UNet"
    if name == "controlnet":
        with pytest.raises(NotImplementedError, match="PAG with ControlNet residuals"):
            pipe(pag_scale=3.0)
    if name == "inpaint":
        with pytest.raises(NotImplementedError, match="PAG with ControlNet residuals"):
            pipe(pag_scale=3.0, down_block_res_samples=[torch.zeros(1)], mid_block_res_sample=torch.zeros(1))
    assert pipe.unet.enabled == []


def test_pag_scale_without_enable_pag_selects_the_default():
    pipe = _pipes()["sd15"](_StubUNet(), use_graph=False)
    assert pipe._check_pag(0.0, 0.0) == dict(pag_scale=0.0, pag_adaptive_scale=0.0) and pipe.unet.enabled == []
    assert pipe._check_pag(2.5, 0.001) == dict(pag_scale=2.5, pag_adaptive_scale=0.001)
    assert pipe.unet.enabled == [("mid",)] and pipe.unet.pag_layers == ("mid_block.attentions.0.transformer_blocks.0",)
    pipe.enable_pag("down.block_0")
    pipe._check_pag(2.5, 0.0)
    assert pipe.unet.pag_layers == ("down_blocks.0.attentions.0.transformer_blocks.0",), "a selection made by hand stays"


def test_engine_refuses_before_any_launch():
    """DenoiseEngine.run itself (callers that bypass the pipelines): the same two combinations, named, before it touches
    its UNet's device -- the stub has none"""
    from consistentid_amd.denoise import DenoiseEngine
    unet = _StubUNet()
    eng = DenoiseEngine(unet, S.DDIMScheduler(), use_graph=False)
    lat, e = torch.zeros(1, 4, 8, 8), torch.zeros(1, 81, 128)
    kw = dict(num_inference_steps=4, guidance_scale=5.0, start_merge_step=1)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        eng.run(lat, e, e, e, pag_scale=3.0, guidance_rescale=0.7, **kw)
    for extra in (dict(controlnet=object()), dict(down_residuals=[lat], mid_residual=lat)):
        with pytest.raises(NotImplementedError, match="PAG with ControlNet residuals"):
            eng.run(lat, e, e, e, pag_scale=3.0, **extra, **kw)
    with pytest.raises(ValueError, match="pag_scale"):
        eng.run(lat, e, e, e, pag_scale=-1.0, **kw)
    with pytest.raises(ValueError, match="pag_adaptive_scale"):
        eng.run(lat, e, e, e, pag_scale=1.0, pag_adaptive_scale=float("nan"), **kw)
    assert unet.enabled == []


def test_unet_forward_refuses_perturbed_rows_it_cannot_serve():
    from consistentid_amd.unet import HipUNet
    hip = HipUNet.__new__(HipUNet)
    hip.config, hip.W, hip._pag = U.tiny_config("sd15"), {}, ()
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="enable_pag"):
        hip.forward_tokens(x, None, None, 3, pag_rows=1)
    hip._pag = ("mid_block.attentions.0.transformer_blocks.0",)
    for rows in (-1, 4):
        with pytest.raises(ValueError, match="pag_rows"):
            hip.forward_tokens(x, None, None, 3, pag_rows=rows)
    with pytest.raises(NotImplementedError, match="PAG with ControlNet residuals"):
        hip.forward_tokens(x, None, None, 3, down_residuals=[x], mid_residual=x, pag_rows=1)


# ----------------------------------------------------------------------------------------------------------- the C ABI
def test_entries_are_declared_exported_and_bound(lib):
    from consistentid_amd import _lib, ops
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", (ROOT / "include" / "cid.h").read_text()))
    assert set(ENTRIES) <= names
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"libcid.so does not export {n}"
    assert lib.cid_version() >= 114
    assert callable(ops.cfg_pag_ddim_step) and callable(ops.cfg_pag_multistep_step) and callable(ops.pag_multistep_step)


P = 4096        # a 16-byte-aligned stand-in address: every call below is refused before anything is launched


def _ddim(lib, **kw):
    a = {**dict(eps=P, lat=P, coef=P, g=5.0, pag=P, mask=None, init=None, noise=None, B=1, per=16), **kw}
    return lib.cid_cfg_pag_ddim_step_f16(a["eps"], a["lat"], a["coef"], a["g"], a["pag"], a["mask"], a["init"], a["noise"],
                                         a["B"], a["per"], None)


def _multistep(lib, cfg):
    def call(**kw):
        a = {**dict(eps=P, lat=P, hist=P, saved=P, z=None, z_rows=0, row=P, g=5.0, pag=P, mask=None, init=None, noise=None,
                    B=1, per=16), **kw}
        head = (a["eps"], a["lat"], a["hist"], a["saved"], a["z"], a["z_rows"], a["row"])
        tail = (a["pag"], a["mask"], a["init"], a["noise"], a["B"], a["per"], None)
        if cfg:
            return lib.cid_cfg_pag_multistep_step_f16(*head, a["g"], *tail)
        return lib.cid_pag_multistep_step_f16(*head, *tail)
    return call


def _common_refusals(lib, call, pointers):
    err = lib.cid_last_error
    for name in pointers + ("pag",):
        assert call(**{name: None}) == -22 and b"null pointer" in err(), name
    assert call(mask=P) == -22 and b"mask/init/noise" in err()
    assert call(mask=P, init=P) == -22 and call(init=P, noise=P) == -22
    for B in (0, -1):
        assert call(B=B) == -22 and b"multiple of 8" in err()
    assert call(per=0) == -22 and call(per=-8) == -22
    assert call(B=1, per=12) == -22 and b"multiple of 8" in err()
    assert call(B=3, per=4) == -22


def test_ddim_entry_refuses_bad_arguments(lib):
    """what cid_cfg_ddim_step_f16 refuses, and a null pag"""
    _common_refusals(lib, lambda **kw: _ddim(lib, **kw), ("eps", "lat", "coef"))


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "single-pass"])
def test_multistep_entries_refuse_bad_arguments(lib, cfg):
    """each entry refuses what its own sibling refuses, and a null pag"""
    call = _multistep(lib, cfg)
    _common_refusals(lib, call, ("eps", "lat", "hist", "saved", "row"))
    assert call(z=P, z_rows=0) == -22 and call(z=None, z_rows=2) == -22 and call(z=P, z_rows=-1) == -22
    assert b"z and z_rows" in lib.cid_last_error()
    assert (b"cid_cfg_pag_multistep_step_f16" if cfg else b"cid_pag_multistep_step_f16") in lib.cid_last_error()
    if not cfg:     # the single-pass sibling, cid_multistep_step_f16, also refuses misaligned buffers (tests/test_lcm_host.py)
        for name in ("eps", "lat", "hist", "saved", "row"):
            assert call(**{name: P + 8}) == -22 and b"16-byte aligned" in lib.cid_last_error(), name
        assert call(z=P + 2, z_rows=1) == -22 and b"16-byte aligned" in lib.cid_last_error()
        for name in ("mask", "init", "noise"):
            assert call(**{"mask": P, "init": P, "noise": P, name: P + 4}) == -22 and b"16-byte aligned" in lib.cid_last_error()
