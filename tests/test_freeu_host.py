"""FreeU without a GPU: the closed form cid_freeu_f16 evaluates against the torch.fft statement of diffusers' fourier_filter
in float64; enable_freeu / disable_freeu on the four pipelines and their argument checks; cid_freeu_f16 is declared, exported
and bound and refuses bad arguments on the host; the workspace query and the slicing rule behind it."""
import re
from pathlib import Path

import pytest
import torch

from freeu_ref import apply_freeu, closed_form, fourier_filter

ROOT = Path(__file__).resolve().parents[1]
SIZES = [(2, 2), (2, 3), (3, 5), (8, 8), (16, 16), (17, 32), (27, 36), (54, 72), (64, 64)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_closed_form_is_the_fourier_filter(hw):
    """threshold = 1 leaves the frequencies {-1, 0}^2 in the box, on even and odd sides alike: seven real sums per plane"""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64) + 0.7
    for s in (0.2, 0.9, 1.0, 1.4):
        ref = fourier_filter(x, 1, s)
        got = closed_form(x, s)
        err = float((got - ref).abs().max())
        assert err <= 1e-13, (hw, s, err)
    assert torch.equal(closed_form(x, 1.0), x)


def test_apply_freeu_touches_the_first_two_blocks_only():
    g = torch.Generator().manual_seed(1)
    h, k = torch.randn(1, 8, 4, 4, generator=g, dtype=torch.float64), torch.randn(1, 4, 4, 4, generator=g, dtype=torch.float64)
    h0, k0 = apply_freeu(0, h, k, 0.9, 0.2, 1.2, 1.4)
    assert torch.equal(h0[:, :4], h[:, :4] * 1.2) and torch.equal(h0[:, 4:], h[:, 4:]) and torch.equal(k0, fourier_filter(k, 1, 0.9))
    h1, k1 = apply_freeu(1, h, k, 0.9, 0.2, 1.2, 1.4)
    assert torch.equal(h1[:, :4], h[:, :4] * 1.4) and torch.equal(k1, fourier_filter(k, 1, 0.2))
    h2, k2 = apply_freeu(2, h, k, 0.9, 0.2, 1.2, 1.4)
    assert h2 is h and k2 is k


def test_every_pipeline_has_enable_and_disable_freeu():
    from consistentid_amd import pipeline
    for cls in (pipeline.ConsistentIDStableDiffusionPipeline, pipeline.ConsistentIDStableDiffusionXLPipeline,
                pipeline.StableDiffusionInpaintConsistentIDPipeline, pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline):
        assert callable(getattr(cls, "enable_freeu", None)) and callable(getattr(cls, "disable_freeu", None)), cls.__name__


class _UNetStub:
    def __init__(self):
        self.calls = []

    def enable_freeu(self, *a):
        self.calls.append(a)

    def disable_freeu(self):
        self.calls.append("off")


def test_enable_freeu_argument_validation():
    """diffusers' positional order (s1, s2, b1, b2); all four required, finite numbers; the UNet is not told of a bad call"""
    from consistentid_amd import pipeline
    cls = pipeline.ConsistentIDStableDiffusionPipeline
    pipe = cls.__new__(cls)
    pipe.unet = _UNetStub()
    pipe.enable_freeu(0.9, 0.2, 1.2, 1.4)
    pipe.enable_freeu(s1=1, s2=0.5, b1=1.5, b2=2)
    pipe.disable_freeu()
    assert pipe.unet.calls == [(0.9, 0.2, 1.2, 1.4), (1.0, 0.5, 1.5, 2.0), "off"]
    assert all(isinstance(v, float) for v in pipe.unet.calls[1])
    for bad in (float("nan"), float("inf"), -float("inf"), None, "0.9", True, [0.9], 1 + 0j):
        for k in range(4):
            args = [0.9, 0.2, 1.2, 1.4]
            args[k] = bad
            with pytest.raises(ValueError, match=("s1", "s2", "b1", "b2")[k]):
                pipe.enable_freeu(*args)
    with pytest.raises(TypeError):
        pipe.enable_freeu(0.9, 0.2, 1.2)
    assert len(pipe.unet.calls) == 3


def test_unet_switch_moves_the_epoch_only_on_a_change():
    """the four values are launch scalars inside captured step graphs: every change re-keys them (denoise.captured_reads
    holds the epoch), a repeated call does not"""
    from consistentid_amd.unet import HipUNet
    u = HipUNet.__new__(HipUNet)
    u.epoch, u._freeu = 0, None
    u.disable_freeu()
    assert (u.epoch, u._freeu) == (0, None)
    u.enable_freeu(0.9, 0.2, 1.2, 1.4)
    assert (u.epoch, u._freeu) == (1, (0.9, 0.2, 1.2, 1.4))
    u.enable_freeu(0.9, 0.2, 1.2, 1.4)
    assert u.epoch == 1
    u.enable_freeu(0.9, 0.2, 1.2, 1.5)
    assert u.epoch == 2
    u.disable_freeu()
    assert (u.epoch, u._freeu) == (3, None)


def test_symbol_is_declared_exported_and_bound(lib):
    from consistentid_amd import _lib
    src = (ROOT / "include" / "cid.h").read_text()
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", src))
    for n in ("cid_freeu_f16", "cid_freeu_ws_bytes"):
        assert n in names and n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.cid_version() >= 109


def _refused(lib, rc, fragment):
    msg = lib.cid_last_error()
    assert rc == -22 and fragment in msg, (rc, msg)


def test_freeu_refuses_bad_arguments_without_launching(lib):
    """every refusal is -22 with a message, decided on the host: the addresses are fake and no GPU is present"""
    A = 4096

    def call(x=A, c_x=32, b=1.2, skip=A, out=A, c_skip=16, s=0.9, B=1, H=4, W=4, ws=A):
        return lib.cid_freeu_f16(x, c_x, b, skip, out, c_skip, s, B, H, W, ws, None)

    for kw in (dict(x=None), dict(skip=None), dict(out=None), dict(ws=None)):
        _refused(lib, call(**kw), b"cid_freeu_f16: null pointer")
    for B in (0, -1, 65536):
        _refused(lib, call(B=B), b"cid_freeu_f16: B must be in 1..65535")
    for H, W in ((1, 8), (8, 1), (1, 1), (0, 4), (4, -2), (1025, 4), (4, 1025)):
        _refused(lib, call(H=H, W=W), b"cid_freeu_f16: H and W must be in 2..1024")
    for c_x in (0, -16, 8, 24, 40, 1288):
        _refused(lib, call(c_x=c_x), b"cid_freeu_f16: c_x must be a positive multiple of 16")
    for c_skip in (0, -8, 4, 12, 321):
        _refused(lib, call(c_skip=c_skip), b"cid_freeu_f16: c_skip must be a positive multiple of 8")
    for kw in (dict(x=A + 8), dict(skip=A + 2), dict(out=A + 4)):
        _refused(lib, call(**kw), b"cid_freeu_f16: x, skip and skip_out must be 16-byte aligned")
    for bad in (float("nan"), float("inf"), -float("inf")):
        _refused(lib, call(s=bad), b"cid_freeu_f16: s and b must be finite")
        _refused(lib, call(b=bad), b"cid_freeu_f16: s and b must be finite")


def test_workspace_query_follows_the_grid_rule(lib):
    """7 x 64 fp32 per (sample, 64-channel slab, token slice); one slice where samples x slabs reach 256 workgroups, otherwise
    enough slices of at least 64 tokens to get there -- and never more than H = W = 1024 asks for"""
    from consistentid_amd import ops
    per = 7 * 64 * 4
    assert ops.freeu_ws_bytes(8, 1280, 8, 8) == 8 * 20 * 1 * per          # 160 workgroups, 64 tokens: one slice
    assert ops.freeu_ws_bytes(8, 1280, 16, 16) == 8 * 20 * 2 * per        # ... 256 tokens: two slices -> 320 workgroups
    assert ops.freeu_ws_bytes(16, 1280, 32, 32) == 16 * 20 * per          # 320 workgroups already
    assert ops.freeu_ws_bytes(2, 320, 64, 64) == 2 * 5 * 26 * per         # SDXL up block 1: 10 -> 260 workgroups
    assert ops.freeu_ws_bytes(1, 320, 64, 64) == 5 * 52 * per
    assert ops.freeu_ws_bytes(1, 8, 2, 2) == per                          # the smallest legal case: one slab, one slice
    assert ops.freeu_ws_bytes(3, 24, 5, 3) == 3 * per
    for B, c in ((1, 8), (2, 320), (2, 640), (8, 1280), (3, 24), (40, 640)):
        top = ops.freeu_ws_bytes(B, c, 1024, 1024)
        for hw in SIZES + [(128, 128), (96, 80), (1024, 2)]:
            assert 0 < ops.freeu_ws_bytes(B, c, *hw) <= top
    for bad in ((0, 8, 4, 4), (1, 0, 4, 4), (1, 8, 0, 4), (1, 8, 4, 1025)):
        assert ops.freeu_ws_bytes(*bad) == 0


def test_front_end_refuses_bad_shapes_before_loading_a_launch(lib):
    """c_x % 16, c_skip % 8, H < 2 or W < 2 and element counts that do not fit: CidError from ops.freeu itself, before it looks
    at where the tensors live; then CPU tensors of a good shape are refused like everywhere else"""
    from consistentid_amd import ops
    from consistentid_amd._lib import CidError
    t = lambda n: torch.zeros(n, dtype=torch.float16)
    ws = torch.zeros(7 * 64, dtype=torch.float32)
    good = dict(B=1, H=2, W=2, c_x=16, c_skip=8, s=0.9, b=1.2)
    for kw, frag in ((dict(c_x=24), "c_x = 24"), (dict(c_x=8), "c_x = 8"), (dict(c_skip=12), "c_skip = 12"), (dict(c_skip=0), "c_skip = 0"),
                     (dict(H=1), "1 x 2"), (dict(W=1), "2 x 1"), (dict(H=0), "0 x 2")):
        a = {**good, **kw}
        with pytest.raises(CidError, match=frag):
            ops.freeu(t(a["B"] * a["H"] * a["W"] * a["c_x"]), t(a["B"] * a["H"] * a["W"] * a["c_skip"]), ws, **a)
    with pytest.raises(CidError, match="elements"):
        ops.freeu(t(64), t(40), ws, **good)
    with pytest.raises(CidError, match="elements"):
        ops.freeu(t(64), t(32), ws, out=t(24), **good)
    with pytest.raises(CidError, match="must live on the GPU"):
        ops.freeu(t(64), t(32), ws, **good)


def test_install_freeu_hooks_the_first_two_up_blocks():
    """the hooked tiny oracle differs from the plain one, and removing the hooks restores it bit for bit"""
    from consistentid_amd import synth
    from freeu_ref import install_freeu
    from oracle_utils import build_oracle, make_weights
    cfg, sd, ad = make_weights("tiny", rank=8)
    oracle = build_oracle("tiny", sd, ad, rank=8)
    inp = synth.random_inputs(cfg, 1, cfg.sample_size * 8, cfg.sample_size * 8)
    run = lambda: oracle(inp["latents"].float(), 501, inp["text"].float()).sample
    with torch.no_grad():
        plain = run()
        handles = install_freeu(oracle, 0.9, 0.2, 1.2, 1.4)
        assert len(handles) == sum(len(b.resnets) for b in oracle.up_blocks[:2])
        hooked = run()
        for h in handles:
            h.remove()
        again = run()
    assert torch.equal(again, plain)
    assert float((hooked - plain).norm() / plain.norm()) > 0.02
