"""The transformer block at the models' real widths, one case per launch-path combination (tests/transformer_paths.py,
tests/golden/transformer_paths.json): which kernels ``HipUNet._transformer`` / ``HipUNet.cross_attention`` launch, with which
weights, buffers and pitches, depends on (channels, heads, context, B, Bp, H, W) -- a wrong operand for one combination is
invisible to the kernel tests and to the toy UNets, which run the first-generation fused kernel everywhere.

Engines: a two-level UNet (or ControlNet encoder) with one real-width attention level, one per (family, width).  A case
calls ``_transformer`` on the first down block's transformer (the CFG-deduplicated cases: the whole forward, traced inside
that transformer only) and asserts
  * the launches are the combination the case is filed under (``observed(trace) == predict(shape) ==`` the table's row);
  * parity with the oracle's own ``Transformer2DModel`` in fp32 on the CPU, held to the oracle's fp16 arm on the GPU
    (conftest.check_vs_fp16_arm at its default slack);
  * a finite output that differs from the input, the same bits on a second call, B * H * W rows whatever the padding.

The rows under "long" run the same case at 154 + 4, 231 + 4 and 158 + 0 context rows and, at 1280 channels, at 1024 text rows:
every layer on the long-context core (csrc/xattn_long.hip) between ``attn2.wql`` or ``norm2`` + ``attn2.wq`` and the out
projection, which writes at pitch 5c where the tail is folded; ``cross_attention_path`` must name what ran.  They follow the
short rows of their width, so one engine's K/V buffers grow from 81 to 158 to 1028 rows."""
import dataclasses
import gc

import pytest
import torch

import transformer_paths as tp
from conftest import check_vs_fp16_arm, half_arm
from oracle_utils import build_oracle, make_weights

pytestmark = pytest.mark.gpu
BLOCK = "down_blocks.0.attentions.0"
CASES = tp.ordered_cases(tp.load())         # a width's long-context rows behind its short ones: one engine serves both


def _overrides(c, heads, n_layers):
    return dict(block_out_channels=(c, c), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), transformer_layers_per_block=(n_layers, n_layers),
                num_attention_heads=(heads, heads))


class _Engine:
    """the HIP engine, the oracle's block in fp32 on the CPU and in fp16 on the GPU, the whole oracle where a case needs it"""

    def __init__(self, dev, family, c, heads, n_layers):
        over = _overrides(c, heads, n_layers)
        if family == "controlnet":
            from consistentid_amd import synth, unet_spec
            from consistentid_amd.controlnet import HipControlNet
            from oracle import unet as ounet
            from oracle.controlnet import ControlNetModel
            cfg = dataclasses.replace(unet_spec.sd15_config(), **over)
            sd = synth.random_controlnet_state_dict(cfg, seed=4, device=dev)
            self.hip = HipControlNet(cfg, sd, device=dev)
            oracle = ControlNetModel(dataclasses.replace(ounet.sd15_config(), **over))
            oracle.load_state_dict({k: v.detach().cpu().float() for k, v in sd.items()}, strict=True)
            oracle.eval()
        else:
            from consistentid_amd.unet import HipUNet
            cfg, sd, ad = make_weights(family, rank=8, device=dev, **over)
            self.hip = HipUNet(cfg, sd, ad, device=dev)
            oracle = build_oracle(family, sd, ad, rank=8, **over)
        self.cfg = cfg
        self.block32 = oracle.down_blocks[0].attentions[0]
        self.block16 = half_arm(self.block32, dev)
        dedup = family == "sd15" and c == 320           # the only transformer a CFG batch reaches deduplicated
        self.oracle32 = oracle if dedup else None
        self.oracle16 = half_arm(oracle, dev) if dedup else None
        self.spec = self.hip.downs[0].attentions[0]
        assert self.spec.name == BLOCK and (self.spec.channels, self.spec.heads, self.spec.n_layers) == (c, heads, n_layers)


@pytest.fixture(scope="module")
def engines(dev):
    held = {}

    def get(family, c, heads, n_layers):
        if (family, c) not in held:         # the cases come family by family, width by width: one engine alive at a time
            held.clear()
            gc.collect()
            torch.cuda.empty_cache()
            held[(family, c)] = _Engine(dev, family, c, heads, n_layers)
        return held[(family, c)]
    yield get
    held.clear()


def _check_launches(tr, shp, comb, hip):
    got, want = tp.observed(tr), tp.predict(*shp)
    assert got == want == comb, f"launched {dict(zip(tp.FIELDS, got))}, predicted {dict(zip(tp.FIELDS, want))}, filed under {comb}"
    c, heads, n_layers, n_txt, n_ip, B, Bp, H, W = shp
    if tp.long_context(n_txt, n_ip):        # what the engine says it runs is what it ran
        assert (hip._ctx.n_txt, hip._ctx.n_ip) == (n_txt, n_ip)
        launches = {"long+fold": "(three launches)", "long": "(four launches)"}[got[3]]
        for k in range(n_layers):
            path = hip.cross_attention_path(f"{BLOCK}.transformer_blocks.{k}", c, B, tp.padded_tokens(c, heads, n_txt, n_ip, H, W))
            assert f"id_xattn_long core<{n_txt},{n_ip}>" in path and path.endswith(launches), (path, got[3])


def _block_case(dev, eng, family, shp, comb):
    c, heads, n_layers, n_txt, n_ip, B, Bp, H, W = shp
    hip, N = eng.hip, H * W
    g = torch.Generator().manual_seed(1000 * B + N)
    x = torch.randn(B * N, c, generator=g)
    x[::4] += 2.0                                       # every fourth token row off centre: the LayerNorm folds see an offset
    x = x.half()
    R = B + 1                                           # one context row more than samples ...
    ehs = torch.randn(R, n_txt + n_ip, eng.cfg.cross_attention_dim, generator=g).half()
    rows = [R - 1 - i for i in range(B)]                # ... read through a selector that is no identity and repeats a row
    if B > 1:
        rows[-1] = rows[0]
    hip.set_context(ehs.to(dev))
    kvrow = torch.tensor(rows, dtype=torch.int32, device=dev)
    xd = x.to(dev)
    with tp.Trace(B, Bp, H, W) as tr:
        out = hip._transformer(eng.spec, xd, B, H, W, kvrow)
    again = hip._transformer(eng.spec, xd, B, H, W, kvrow)
    torch.cuda.synchronize()
    _check_launches(tr, shp, comb, hip)
    assert out.shape == (B * N, c), f"{tuple(out.shape)} for {B} x {N} tokens"
    assert torch.equal(out, again), "a second call gives other bits"
    assert torch.isfinite(out.float()).all() and (out.float() - xd.float()).abs().max() > 1e-2
    nchw = lambda t: t.view(B, H, W, c).permute(0, 3, 1, 2)
    with torch.no_grad():
        ref = eng.block32(nchw(x.float()), ehs[rows].float())
        arm = eng.block16(nchw(xd), ehs.to(dev)[rows])
    return check_vs_fp16_arm(nchw(out), ref, arm, tp.case_id(family, shp))


def _dedup_case(dev, eng, family, shp, comb):
    c, heads, n_layers, n_txt, n_ip, B, Bp, H, W = shp
    hip, rep, t = eng.hip, B // Bp, 481
    g = torch.Generator().manual_seed(1000 * B + H * W)
    lat = torch.randn(Bp, eng.cfg.in_channels, H, W, generator=g).half()
    ehs = torch.randn(B, n_txt + n_ip, eng.cfg.cross_attention_dim, generator=g).half()
    hip.set_context(ehs.to(dev))
    kvrow = torch.arange(B, dtype=torch.int32, device=dev)
    hip._t_buf.fill_(float(t))
    with tp.Trace(B, Bp, H, W) as tr, tr.only(hip, BLOCK):
        out = hip.forward_tokens(lat.to(dev), hip._t_buf, kvrow, B)
    x, y = tr.block_in, tr.block_out
    again = hip.forward_tokens(lat.to(dev), hip._t_buf, kvrow, B)
    torch.cuda.synchronize()
    _check_launches(tr, shp, comb, hip)
    assert x.shape == (Bp * H * W, c) and y.shape == (B * H * W, c), (tuple(x.shape), tuple(y.shape))
    assert torch.equal(out, again), "a second call gives other bits"
    assert torch.isfinite(y.float()).all() and (y.float() - x.float().repeat(rep, 1)).abs().max() > 1e-2
    lat_b = torch.cat([lat] * rep)
    with torch.no_grad():
        ref = eng.oracle32(lat_b.float(), t, ehs.float()).sample
        arm = eng.oracle16(lat_b.to(dev), t, ehs.to(dev)).sample
    return check_vs_fp16_arm(out, ref, arm, tp.case_id(family, shp))


@pytest.mark.parametrize("family,shp,comb", CASES, ids=[tp.case_id(f, s) for f, s, _ in CASES])
def test_transformer_path(dev, engines, family, shp, comb):
    eng = engines(family, *shp[:3])
    e, e_arm = (_dedup_case if shp[5] != shp[6] else _block_case)(dev, eng, family, shp, comb)
    print(f"[paths] {tp.case_id(family, shp)}: ours / arm = {e / max(e_arm, 1e-30):.3f}")
