"""HIP execution engine for the ControlNet encoder.

Drop-in for the object the reference's ControlNet-inpaint pipeline calls as
``self.controlnet(control_model_input, t, encoder_hidden_states=controlnet_prompt_embeds,
controlnet_cond=control_image, conditioning_scale=cond_scale, return_dict=False)``
(pipelines/StableDIffusionControlNetInpaint_ConsistentID.py:405-412; the model is diffusers'
``ControlNetModel`` loaded at demo/controlnet_demo.py:44-47).

It is the UNet's encoder half with diffusers' DEFAULT attention (the reference installs the
ConsistentID processors on the UNet only): all 81 context tokens are keys of ONE softmax, which the
fused cross-attention kernel runs as "n_txt = 81, n_ip = 0".  Everything reuses the UNet engine's
kernels; new here are the condition embedding (small-channel direct convs, computed once per control
image -- it does not depend on the latents or the timestep) and the 1x1 "zero convs" (plain GEMMs).

``HipMultiControlNet`` is diffusers' ``MultiControlNetModel`` over 1..4 such engines (the reference keeps that class's
branches: CN :139-149 guidance windows per net, :281-301 one control image per net, :363-370 a keep list per net and step,
:397-398 ``cond_scale = [c * s for c, s in zip(controlnet_conditioning_scale, controlnet_keep[i])]``): the nets run
one after another with UNSCALED zero convs and cid_residual_accum_f16 sums their residuals, scaled from a device vector.
The window / scale bookkeeping of those reference lines is in the pure functions below (no GPU needed).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import MAX_CONTROLNETS
from .unet import HipUNet
from .unet_spec import UNetConfig


def check_controlnet_count(n: int) -> int:
    """1..MAX_CONTROLNETS (CID_MAX_CONTROLNETS, include/cid.h): the nets one cid_residual_accum_f16 launch sums"""
    if not 1 <= n <= MAX_CONTROLNETS:
        raise ValueError(f"{n} ControlNets: a MultiControlNet takes 1..{MAX_CONTROLNETS}")
    return n


def broadcast_conditioning_scale(scale, n_nets: int) -> List[float]:
    """``controlnet_conditioning_scale`` -> one float per net.  A float is repeated, as diffusers' own ControlNet pipelines
    do (``[scale] * len(nets)``); the reference does not and would fail in its ``zip`` (CN :398) on a float."""
    if isinstance(scale, (list, tuple)):
        if len(scale) != n_nets:
            raise ValueError(f"controlnet_conditioning_scale has {len(scale)} entries for {n_nets} ControlNets")
        return [float(s) for s in scale]
    return [float(scale)] * n_nets


def align_control_guidance(start, end, n_nets: int) -> Tuple[List[float], List[float]]:
    """``control_guidance_start`` / ``control_guidance_end`` -> two lists of ``n_nets`` floats, as CN :139-149 aligns them:
    a float beside a list is repeated to the list's length, two floats to the number of nets.  (Tuples count as lists.)"""
    start = list(start) if isinstance(start, tuple) else start
    end = list(end) if isinstance(end, tuple) else end
    if not isinstance(start, list) and isinstance(end, list):
        start = len(end) * [start]
    elif not isinstance(end, list) and isinstance(start, list):
        end = len(start) * [end]
    elif not isinstance(start, list) and not isinstance(end, list):
        start, end = n_nets * [start], n_nets * [end]
    if len(start) != len(end):
        raise ValueError(f"control_guidance_start has {len(start)} entries, control_guidance_end has {len(end)}")
    if len(start) != n_nets:
        raise ValueError(f"control_guidance_start / control_guidance_end have {len(start)} entries for {n_nets} ControlNets")
    return [float(s) for s in start], [float(e) for e in end]


def controlnet_keep_table(n_steps: int, starts: Sequence[float], ends: Sequence[float], first_step: int = 0) -> List[List[float]]:
    """CN :363-370: ``keep[i][k] = 1.0 - float(i / n < start_k or (i + 1) / n > end_k)`` over the ``n_steps`` executed
    steps; ``first_step`` rows of zeros stand in front for the schedule entries a ``strength`` < 1 window skips (the
    reference enumerates the truncated timestep list, so its i = 0 is schedule entry ``first_step``)."""
    rows = [[0.0] * len(starts) for _ in range(first_step)]
    for i in range(n_steps):
        rows.append([1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in zip(starts, ends)])
    return rows


def active_nets(keep_row: Sequence[float]) -> Tuple[int, ...]:
    """the nets that run in a step: keep > 0 (the others' residuals are scaled by 0 there, CN :397-398)"""
    return tuple(k for k, v in enumerate(keep_row) if v > 0.0)


def prepare_control_arguments(controlnet, control_image, conditioning_scale, guidance_start, guidance_end, size) -> dict:
    """The ControlNet arguments of the pipeline's ``__call__`` -> the denoise engine's ``controlnet``, ``control_image``,
    ``conditioning_scale``, ``control_guidance_start`` and ``control_guidance_end``.  ``controlnet`` is the pipeline's: a
    ``HipMultiControlNet`` takes one control image per net (CN :281-301), scales broadcast and windows aligned as CN
    :139-149; a plain ``HipControlNet`` (or none) goes the same way as a list of one -- of a list it reads the first
    scale and window (CN :352-358, :399-402) -- and is unwrapped at the end.  PIL images are resized to ``size`` =
    (height, width).  Without a ``control_image`` no net runs (``controlnet`` None)."""
    from . import image_prep
    multi = isinstance(controlnet, HipMultiControlNet)
    n_nets = len(controlnet.nets) if multi else 1
    if multi:
        scales = broadcast_conditioning_scale(conditioning_scale, n_nets)
        starts, ends = align_control_guidance(guidance_start, guidance_end, n_nets)
    else:
        scales, starts, ends = ([float(v[0] if isinstance(v, (list, tuple)) else v)] for v in
                                (conditioning_scale, guidance_start, guidance_end))
    images = None
    if control_image is not None:
        if controlnet is None:
            raise ValueError("control_image given but the pipeline was built without a controlnet")
        several = isinstance(control_image, (list, tuple))
        if not multi and several and len(control_image) > 1:
            raise NotImplementedError("MultiControlNet: several control images need a pipeline built with a list of "
                                      "ControlNets (controlnet=[...] / HipMultiControlNet), this one has a single one")
        images = list(control_image) if multi and several else [control_image]
        if len(images) != n_nets:
            raise ValueError(f"control_image has {len(images)} entries for {n_nets} ControlNets")
        for k, item in enumerate(images):                                                  # CN :281-301
            what = f"control_image[{k}]" if multi else "control_image"
            if image_prep.is_pil(item):
                if isinstance(item, (list, tuple)) and len(item) > 1:
                    raise NotImplementedError(f"{what}: one PIL image per ControlNet (got {len(item)})")
                item = image_prep.preprocess_control(item, *size)
            if not torch.is_tensor(item):
                raise NotImplementedError(f"{what}: one PIL image (resized by image_prep.py) or a float tensor "
                                          "[B, 3, 8h, 8w] in [0, 1]; numpy arrays are not taken")
            images[k] = item
    if not multi:
        images, scales, starts, ends = (v[0] if v else None for v in (images, scales, starts, ends))
    return dict(controlnet=None if images is None else controlnet, control_image=images, conditioning_scale=scales,
                control_guidance_start=starts, control_guidance_end=ends)


def _refuse_unbuilt(guess_mode: bool, return_dict: bool):
    if guess_mode:
        raise NotImplementedError("guess_mode residual scaling (the reference never forwards it, CN :405-412)")
    if return_dict:
        raise NotImplementedError("return_dict=True (the reference passes return_dict=False, CN :411)")


def _nchw(down, mid, B: int, shapes):
    """token-major residuals [B * h * w, c] -> (down, mid) as [B, c, h, w]-shaped (channels-last) views; ``shapes``: (c, h, w)
    of every down residual, then of the mid one"""
    view = lambda t, s: t.view(B, s[1], s[2], s[0]).permute(0, 3, 1, 2)
    return [view(t, s) for t, s in zip(down, shapes[:-1])], view(mid, shapes[-1])


class HipControlNet(HipUNet):
    def __init__(self, cfg: UNetConfig, controlnet_sd: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0",
                 packed=None):
        super().__init__(cfg, controlnet_sd, None, device, num_tokens=0, packed=packed, encoder_only=True)
        self._cond_key = None
        self._cond_ref = None
        self._cond_emb: Optional[torch.Tensor] = None
        self._scaled: Dict[float, Dict[str, torch.Tensor]] = {}

    # ------------------------------------------------------------------ condition embedding (once per image)
    def cond_embedding(self, controlnet_cond: torch.Tensor) -> torch.Tensor:
        """[B, 3, 8h, 8w] image -> token-major [B * h * w, C0]; cached until the image tensor changes."""
        # (the keyed tensor is kept alive in _cond_ref so that its address cannot be recycled for another image)
        key = (controlnet_cond.data_ptr(), controlnet_cond._version, tuple(controlnet_cond.shape))
        if key == self._cond_key and self._cond_ref is controlnet_cond:
            return self._cond_emb
        W = self.W
        img = controlnet_cond.to(device=self.device, dtype=torch.float16)
        B, cin, H, Wd = img.shape
        x = img.permute(0, 2, 3, 1).reshape(B * H * Wd, cin).contiguous()     # token-major, once per generation
        for name, ci, co, stride, silu in self.packed.cond_convs:
            assert ci == cin, (name, ci, cin)
            Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
            y = self._empty(B * Ho * Wo, co)
            ops.conv3x3_small(x, y, W[f"{name}.w"], W[f"{name}.b"], B=B, Hi=H, Wi=Wd, cin=ci, cout=co,
                              stride=stride, silu=silu)
            x, cin, H, Wd = y, co, Ho, Wo
        self._cond_key, self._cond_emb, self._cond_ref = key, x, controlnet_cond
        self._cond_hw = (H, Wd)
        return x

    def _zero_weights(self, scale: float) -> Dict[str, torch.Tensor]:
        """zero-conv weights with ``conditioning_scale`` folded in (the reference multiplies every residual by it,
        diffusers controlnet.py; one rounding instead of two)"""
        if scale == 1.0:
            return self.W
        if scale not in self._scaled:
            names = [f"controlnet_down_blocks.{i}" for i in range(self.packed.n_zero)] + ["controlnet_mid_block"]
            self._scaled[scale] = {f"{n}.{s}": (self.W[f"{n}.{s}"].float() * scale).half() for n in names for s in "wb"}
        return self._scaled[scale]

    # ------------------------------------------------------------------ forward
    def forward_tokens(self, sample: torch.Tensor, t_dev: torch.Tensor, kvrow: torch.Tensor, B: int,
                       cond_emb: torch.Tensor, conditioning_scale: float = 1.0, temb: Optional[torch.Tensor] = None,
                       in_scale: Optional[torch.Tensor] = None) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """sample [B, 4, h, w] fp16 NCHW; ``cond_emb`` from :meth:`cond_embedding` (B or 1 images).
        Returns the 12 (+1) residuals token-major ``[B * HW_i, C_i]`` -- the layout
        ``HipUNet.forward_tokens(down_residuals=..., mid_residual=...)`` consumes."""
        cfg, W = self.config, self.W
        Bin, cin, H, Wd = sample.shape
        if temb is None:
            temb = self.time_embed(t_dev, B, None)
        trows = temb.shape[0]
        c0 = cfg.block_out_channels[0]
        x = self._empty(B * H * Wd, c0)
        ops.conv_in(sample, x, W["conv_in.w"], W["conv_in.b"], B=B, Bin=Bin, cin=cin, H=H, W=Wd, cout=c0, in_scale=in_scale)
        assert cond_emb.shape[1] == c0 and (B * H * Wd) % cond_emb.shape[0] == 0, "control image must be 8x the latent size"
        ops.add_inplace(x, cond_emb)                        # sample = conv_in(sample) + cond_embedding(cond)
        skips = [(x, c0, H, Wd)]
        c = c0
        for blk in self.downs:
            for j, r in enumerate(blk.resnets):
                x = self._resnet(r, x, None, c, 0, B, H, Wd, temb, trows)
                c = r.cout
                if blk.attentions:
                    x = self._transformer(blk.attentions[j], x, B, H, Wd, kvrow)
                skips.append((x, c, H, Wd))
            if blk.sampler:
                n = f"{blk.name}.{blk.sampler}.conv"
                Ho, Wo = H // 2, Wd // 2
                y = self._empty(B * Ho * Wo, c)
                ops.gemm(x, W[f"{n}.w"], y, M=B * Ho * Wo, N=c, c1=c, bias=W[f"{n}.b"], taps=9,
                         Hi=H, Wi=Wd, Ho=Ho, Wo=Wo, stride=2, ws=self._gemm_ws)
                x, H, Wd = y, Ho, Wo
                skips.append((x, c, H, Wd))
        x = self._resnet(self.mid.resnets[0], x, None, c, 0, B, H, Wd, temb, trows)
        x = self._transformer(self.mid.attentions[0], x, B, H, Wd, kvrow)
        x = self._resnet(self.mid.resnets[1], x, None, c, 0, B, H, Wd, temb, trows)
        Z = self._zero_weights(float(conditioning_scale))
        assert len(skips) == self.packed.n_zero
        down = []
        for i, (s, sc_, sh, sw) in enumerate(skips):
            o = self._empty(B * sh * sw, sc_)
            n = f"controlnet_down_blocks.{i}"
            ops.gemm(s, Z[f"{n}.w"], o, M=B * sh * sw, N=sc_, c1=sc_, bias=Z[f"{n}.b"], ws=self._gemm_ws)
            down.append(o)
        mid = self._empty(B * H * Wd, c)
        ops.gemm(x, Z["controlnet_mid_block.w"], mid, M=B * H * Wd, N=c, c1=c, bias=Z["controlnet_mid_block.b"],
                 ws=self._gemm_ws)
        self._last_shapes = [(sc_, sh, sw) for (_, sc_, sh, sw) in skips] + [(c, H, Wd)]
        return down, mid

    # ------------------------------------------------------------------ diffusers-style call
    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                 guess_mode: bool = False, return_dict: bool = False):
        """Returns ``(down_block_res_samples, mid_block_res_sample)`` as [B, C, H, W]-shaped (channels-last) views,
        which ``HipUNet.__call__`` takes back without a copy."""
        _refuse_unbuilt(guess_mode, return_dict)
        if isinstance(conditioning_scale, (list, tuple)):
            raise NotImplementedError("MultiControlNet: a list of scales goes to HipMultiControlNet([...]), this is one net")
        sample = sample.to(device=self.device, dtype=torch.float16).contiguous()
        B = sample.shape[0]
        self.refresh_context(encoder_hidden_states, num_tokens=0)
        kvrow = torch.arange(B, dtype=torch.int32, device=self.device)
        self._t_buf.fill_(float(timestep))
        cond = self.cond_embedding(controlnet_cond)
        down, mid = self.forward_tokens(sample, self._t_buf, kvrow, B, cond, conditioning_scale)
        return _nchw(down, mid, B, self._last_shapes)


class HipMultiControlNet:
    """diffusers' ``MultiControlNetModel`` over 1..4 ``HipControlNet``s of one geometry (same residual shapes, one device).
    ``nets`` is the list; ``__call__`` follows ``MultiControlNetModel.forward``: every net sees the same sample, timestep and
    encoder_hidden_states with its own control image and scale, and the residuals are summed."""

    def __init__(self, nets):
        nets = list(nets)
        check_controlnet_count(len(nets))
        for k, n in enumerate(nets):
            if not isinstance(n, HipControlNet):
                raise TypeError(f"HipMultiControlNet: entry {k} is {type(n).__name__}, expected HipControlNet")
        geom = lambda n: (n.config.in_channels, tuple(n.config.block_out_channels), tuple(n.config.down_block_types),
                          n.config.layers_per_block, n.config.cross_attention_dim, n.packed.n_zero, str(n.device))
        for k, n in enumerate(nets[1:], 1):
            if geom(n) != geom(nets[0]):
                raise ValueError(f"HipMultiControlNet: net {k} has geometry {geom(n)}, net 0 has {geom(nets[0])} "
                                 "(the residuals of all nets are summed element by element)")
        self.nets = nets
        self.config = nets[0].config
        self.device = nets[0].device
        self._scales = torch.zeros(MAX_CONTROLNETS, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=None,
                 guess_mode: bool = False, return_dict: bool = False):
        """``controlnet_cond`` / ``conditioning_scale``: one control image [B or 1, 3, 8h, 8w] and one float per net.  Returns
        the summed ``(down_block_res_samples, mid_block_res_sample)`` in ``HipControlNet.__call__``'s layout.  The zero
        convs run unscaled and one cid_residual_accum_f16 launch per residual group forms sum_k scale_k * r_k in fp32 with
        one rounding (diffusers rounds every scaled residual and every partial sum to fp16)."""
        _refuse_unbuilt(guess_mode, return_dict)
        N = len(self.nets)
        if not isinstance(controlnet_cond, (list, tuple)) or len(controlnet_cond) != N:
            got = len(controlnet_cond) if isinstance(controlnet_cond, (list, tuple)) else 1
            raise ValueError(f"controlnet_cond has {got} control images for {N} ControlNets")
        scales = broadcast_conditioning_scale(1.0 if conditioning_scale is None else conditioning_scale, N)
        sample = sample.to(device=self.device, dtype=torch.float16).contiguous()
        B = sample.shape[0]
        kvrow = torch.arange(B, dtype=torch.int32, device=self.device)
        downs, mids = [], []
        for net, cond in zip(self.nets, controlnet_cond):
            net.refresh_context(encoder_hidden_states, num_tokens=0)
            net._t_buf.fill_(float(timestep))
            d, m = net.forward_tokens(sample, net._t_buf, kvrow, B, net.cond_embedding(cond), 1.0)
            downs.append(d)
            mids.append(m)
        self._scales.copy_(torch.tensor(scales + [0.0] * (MAX_CONTROLNETS - N), dtype=torch.float32))
        out_d = [torch.zeros_like(t) for t in downs[0]]
        out_m = torch.zeros_like(mids[0])
        ops.residual_accum(out_d, downs, self._scales)
        ops.residual_accum([out_m], [[m] for m in mids], self._scales)
        return _nchw(out_d, out_m, B, self.nets[0]._last_shapes)
