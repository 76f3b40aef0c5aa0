"""FreeU on the GPU: cid_freeu_f16 against float64 (torch.fft, freeu_ref.fourier_filter) on the same fp16 inputs; the tiny
UNets with FreeU against the fp32 oracle with freeu_ref's hooks, within the fp16 arm; one engine with graphs on through
off -> on -> off, bit for bit against fresh eager runs."""
import functools
import math

import pytest
import torch

from conftest import TOL_L2, check_vs_fp16_arm, dev_half, half_arm, rel_l2
from freeu_ref import fourier_filter, install_freeu

pytestmark = pytest.mark.gpu

FREEU = (0.9, 0.2, 1.2, 1.4)        # (s1, s2, b1, b2)

# (B, H, W, c_x, c_skip)
SHAPES = {
    "sd15 up block 0": (2, 8, 8, 1280, 1280),
    "HW = 256": (2, 16, 16, 1280, 640),
    "27 x 36, SDXL 864 x 1152": (1, 27, 36, 1280, 640),
    "64 x 64, token slices": (1, 64, 64, 640, 320),
    "smallest": (1, 2, 2, 16, 8),
    "all odd": (3, 5, 3, 48, 24),
}
CASES = [(k, 0.2, 1.4) for k in SHAPES] + [("27 x 36, SDXL 864 x 1152", 0.9, 1.2)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(x, skip) fp16 on the CPU, token-major.  skip: the smooth plane 1 + cos th + 0.5 sin(th + tw), scaled per channel,
    plus 0.5 randn -- the low band the filter acts on is large"""
    B, H, W, c_x, c_skip = SHAPES[name]
    g = torch.Generator().manual_seed(sum(SHAPES[name]))
    th = (2 * math.pi * torch.arange(H) / H)[:, None]
    tw = (2 * math.pi * torch.arange(W) / W)[None, :]
    plane = 1 + th.cos() + 0.5 * (th + tw).sin()                                    # [H, W]
    amp = torch.linspace(0.5, 2.0, c_skip)
    skip = plane[None, :, :, None] * amp + 0.5 * torch.randn(B, H, W, c_skip, generator=g)
    x = torch.randn(B * H * W, c_x, generator=g)
    return x.half(), skip.reshape(B * H * W, c_skip).half()


@functools.lru_cache(maxsize=None)
def _reference(name, s):
    """float64 fourier_filter of the fp16 skip, token-major, and the mean |x| of every (sample, channel) plane"""
    B, H, W, _, c_skip = SHAPES[name]
    sk = _inputs(name)[1].double().view(B, H, W, c_skip)
    ref = fourier_filter(sk.permute(0, 3, 1, 2), 1, s).permute(0, 2, 3, 1)
    return ref.reshape(B * H * W, c_skip), sk.abs().mean(dim=(1, 2))                # [B, c_skip]


@pytest.mark.parametrize("name,s,b", CASES, ids=[f"{k}, s={s}" for k, s, _ in CASES])
def test_freeu_kernel_vs_float64(dev, name, s, b):
    """per element |got - ref| <= 2^-11 |ref| (one fp16 rounding) + 8 |s - 1| H W 2^-24 mean_plane|x| (the worst case of
    seven fp32 sums over the plane).  Measured on an MI355X: max err / bound 0.45 at 64 x 64 (mean bound 2.5e-3) up to 0.96
    at 8 x 8 (3.6e-4, nearly all of it the rounding term), where the filter itself moves the tensor by 1.0 on average at
    s = 0.2 and by 0.13 at s = 0.9."""
    from consistentid_amd import ops
    B, H, W, c_x, c_skip = SHAPES[name]
    x, skip = _inputs(name)
    ref, plane_abs = _reference(name, s)
    bound = 2.0 ** -11 * ref.abs() + (8 * abs(s - 1) * H * W * 2.0 ** -24 * plane_abs)[:, None, :].expand(B, H * W, c_skip).reshape(ref.shape)
    moved = float((ref - skip.double()).abs().mean())
    print(f"[freeu] {name}, s = {s}: the filter moves the tensor by {moved:.3e} on average, mean bound {float(bound.mean()):.3e}")
    assert moved >= 20 * float(bound.mean())
    ws = torch.zeros(ops.freeu_ws_bytes(B, c_skip, H, W), dtype=torch.uint8, device=dev)
    xd, sd = x.to(dev), skip.to(dev)
    out = torch.full_like(sd, float("nan"))
    ret = ops.freeu(xd, sd, ws, B=B, H=H, W=W, c_x=c_x, c_skip=c_skip, s=s, b=b, out=out)
    torch.cuda.synchronize()
    assert ret is out and torch.equal(sd.cpu(), skip), "out of place: skip itself must stay"
    err = (out.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(f"[freeu] {name}, s = {s}: max err / bound = {worst:.3f}, max |err| = {float(err.max()):.3e}")
    assert torch.isfinite(out.float()).all()
    assert worst <= 1.0, f"{name}: max err / bound = {worst:.3f}"
    # the b half: half(b * x) exactly on the first c_x / 2 channels, the rest untouched
    want = x.clone()
    want[:, :c_x // 2] = (x[:, :c_x // 2].float() * b).half()
    assert torch.equal(xd.cpu().view(torch.int16), want.view(torch.int16))
    # in place gives the same bits as out of place, and a second run the same bits as the first
    x2, s2 = x.to(dev), skip.to(dev)
    s2._gn_stats = ("stale", 64)
    x2._gn_stats = ("stale", 64)
    assert ops.freeu(x2, s2, ws, B=B, H=H, W=W, c_x=c_x, c_skip=c_skip, s=s, b=b) is s2
    torch.cuda.synchronize()
    assert torch.equal(s2.view(torch.int16), out.view(torch.int16)) and torch.equal(x2.view(torch.int16), xd.view(torch.int16))
    assert not hasattr(s2, "_gn_stats") and not hasattr(x2, "_gn_stats"), "the statistics describe the tensors before the update"
    x3, out3 = x.to(dev), torch.empty_like(sd)
    ws.fill_(255)                                   # (NaN patterns: nothing of an earlier run is read)
    ops.freeu(x3, sd, ws, B=B, H=H, W=W, c_x=c_x, c_skip=c_skip, s=s, b=b, out=out3)
    torch.cuda.synchronize()
    assert torch.equal(out3.view(torch.int16), out.view(torch.int16))


def test_freeu_refuses_a_short_workspace(dev):
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    B, H, W, c_x, c_skip = SHAPES["64 x 64, token slices"]
    x, skip = (t.to(dev) for t in _inputs("64 x 64, token slices"))
    ws = torch.zeros(ops.freeu_ws_bytes(B, c_skip, H, W) - 16, dtype=torch.uint8, device=dev)
    with pytest.raises(CidError, match="freeu.ws"):
        ops.freeu(x, skip, ws, B=B, H=H, W=W, c_x=c_x, c_skip=c_skip, s=0.2, b=1.4)


# ----------------------------------------------------------------------------- UNet forward
@pytest.mark.parametrize("name,hw", [("tiny", None), ("tinyxl", None), ("tiny", (96, 80)), ("tinyxl", (96, 80))],
                         ids=["tiny", "tinyxl", "tiny 96x80", "tinyxl 96x80"])
def test_tiny_unet_forward_with_freeu(dev, name, hw, monkeypatch):
    """default latents: up blocks 0 / 1 at 8 x 8 and 16 x 16.  96 x 80 latents: the tiny SD1.5 UNet's up block 0 is at
    24 x 20 = 480 tokens, above GN_SMALL_MAX_HW with sides that are no power of two -- there the resnet's GroupNorm would take
    GEMM-epilogue statistics of the tensors as they were BEFORE FreeU if ops.freeu left them attached."""
    from consistentid_amd import ops, synth
    from consistentid_amd.unet import HipUNet
    from oracle_utils import build_oracle, make_weights
    cfg, sd, ad = make_weights(name, rank=8)
    oracle = build_oracle(name, sd, ad, rank=8)
    hip = HipUNet(cfg, sd, ad, device=dev)
    B = 1 if hw else 2              # (the fp32 oracle runs twice on the CPU: one image at the larger size)
    h, w = hw or (cfg.sample_size, cfg.sample_size)
    inp = synth.random_inputs(cfg, B, 8 * h, 8 * w)
    ehs = torch.cat([inp["null"], inp["text"]])
    kw_o, kw_h = {}, {}
    if name == "tinyxl":
        te = torch.cat([inp["pooled_null"], inp["pooled_text"]])
        kw_o = dict(added_cond_kwargs={"text_embeds": te.float(), "time_ids": inp["time_ids"]})
        kw_h = dict(added_cond_kwargs={"text_embeds": te.to(dev), "time_ids": inp["time_ids"].to(dev)})
    lat2 = torch.cat([inp["latents"]] * 2)
    arm_m = half_arm(oracle, dev)
    run_hip = lambda: hip(lat2.to(dev), 501, encoder_hidden_states=ehs.to(dev), cross_attention_kwargs={}, **kw_h).sample
    with torch.no_grad():
        plain = oracle(lat2.float(), 501, ehs.float(), **kw_o).sample
        install_freeu(oracle, *FREEU)
        install_freeu(arm_m, *FREEU)
        ref = oracle(lat2.float(), 501, ehs.float(), **kw_o).sample
        arm = arm_m(lat2.to(dev).half(), 501, ehs.to(dev).half(), **dev_half(kw_o, dev)).sample
    moved = rel_l2(ref, plain)
    print(f"[freeu] {name} {h} x {w}: FreeU moves the oracle's output by {moved:.3e} relative L2")
    assert moved >= 20 * TOL_L2
    off = run_hip().clone()
    hip.enable_freeu(*FREEU)
    out = run_hip().clone()
    torch.cuda.synchronize()
    check_vs_fp16_arm(out, ref, arm, f"{name} UNet forward with FreeU, {h} x {w} latents")
    # off means no launch: the forward is the one it was, and never reaches ops.freeu
    hip.disable_freeu()

    def boom(*a, **k):
        raise AssertionError("ops.freeu was called with FreeU disabled")
    monkeypatch.setattr(ops, "freeu", boom)
    again = run_hip()
    torch.cuda.synchronize()
    assert torch.equal(again, off) and not torch.equal(out, off)


# ----------------------------------------------------------------------------- engine
def test_engine_rekeys_its_graphs_for_freeu(dev):
    """one pipeline with graphs on: A (off), enable_freeu -> B, disable_freeu -> C.  B is the bits of the same call run
    eagerly on fresh objects with FreeU enabled and differs from A; C is A.  The scalars sit inside the captured launches, so
    both switches must re-capture."""
    from engine_cases import Spec, call_pipeline, executed_steps, new_unet, pipeline_class, product_scheduler
    spec = Spec(steps=4, merge=1, guidance=5.0)
    assert executed_steps(spec) >= 3            # eager, capture, replay
    pipe = pipeline_class(spec)(new_unet(str(dev)), use_graph=True)
    eng = pipe._engine
    a = call_pipeline(pipe, spec, dev)[0].clone()
    n_a = len(eng.captures)
    assert n_a >= 1
    pipe.enable_freeu(*FREEU)
    b = call_pipeline(pipe, spec, dev)[0].clone()
    n_b = len(eng.captures)
    fresh = pipeline_class(spec)(new_unet(str(dev)), scheduler=product_scheduler(spec), use_graph=False)
    fresh.enable_freeu(*FREEU)
    want = call_pipeline(fresh, spec, dev)[0]
    assert not fresh._engine.captures
    assert torch.isfinite(b.float()).all()
    assert torch.equal(b, want), f"graph replay with FreeU differs from the fresh eager run, max |diff| = {(b.float() - want.float()).abs().max():.3e}"
    assert not torch.equal(b, a) and n_b > n_a
    pipe.disable_freeu()
    c = call_pipeline(pipe, spec, dev)[0].clone()
    assert torch.equal(c, a) and len(eng.captures) > n_b
