"""The denoise engine of the four pipelines (pipeline.py): one generation = set_context (K/V of the embed sets) +
S x [ControlNets + UNet(2B) + CFG + scheduler step].  The step is captured once into a hipGraph and replayed; every
per-step host value of the reference's loops lives in one device table (ops.StepTable).

The single pass: under ``LCMScheduler`` with ``guidance_scale <= 1`` -- diffusers'
``do_classifier_free_guidance = guidance_scale > 1`` -- or on a UNet with ``time_cond_proj_dim`` (guidance is in its time
embedding) a step is [ControlNets + UNet(B) on the conditional rows + cid_multistep_step_f16]: no unconditional half and no
CFG combine.  The four other schedulers launch what they always launched at every guidance value.

Perturbed-attention guidance: with ``pag_scale`` > 0 the UNet runs B more rows, the perturbed twins of the
conditional rows, and the step is the ``+pag`` entry of the same kernel with the step's scale read from the step table; with
``pag_scale`` == 0 nothing here changes.

Self-attention guidance: with ``sag_scale`` > 0 a step is [UNet, which also writes the column mass of
the mid block's first self-attention map for the guide rows -> cid_sag_degrade_f16 -> UNet(B) on the degraded latents -> the
``+sag`` entry of the step kernel], still one graph replay; with ``sag_scale`` == 0 nothing here changes.

``DenoiseEngine.run`` is a driver over phases that take and return named values: the static-buffer pool, the graph
cache, the step coefficients (``_StepCoefficients``), the ControlNet plan (``_ControlPlan``), the embed-row selectors
(``step_rows``), what the step reads of objects the engine does not own (``captured_reads``), the step table and the
step closure.

The engine keeps the reference to the ``HipUNet`` it was built on: assigning ``pipe.unet`` afterwards does not reach it (out
of scope; build a new pipeline).  ``pipe.controlnet = other`` and ``pipe.scheduler = other`` take effect on the next call.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import ops
from .controlnet import HipMultiControlNet, active_nets, controlnet_keep_table
from .scheduler import C_IN, DDIMScheduler, LCMScheduler, pack_step_rows, sag_coefficient_table
from .unet import HipUNet


def check_guidance_rescale(guidance_rescale) -> float:
    """``guidance_rescale`` of the reference ``__call__``s (diffusers 0.23 rescale_noise_cfg's phi) -> float; negative or
    non-finite values are refused"""
    phi = float(guidance_rescale)
    if not np.isfinite(phi) or phi < 0.0:
        raise ValueError(f"guidance_rescale = {guidance_rescale!r}: a finite value >= 0 (0 = off, the paper suggests 0.7)")
    return phi


def check_pag(pag_scale, pag_adaptive_scale=0.0) -> tuple:
    """``pag_scale`` / ``pag_adaptive_scale`` of diffusers' PAG pipelines -> two floats; negative or non-finite values (and
    booleans, which are no scales) are refused"""
    for name, v in (("pag_scale", pag_scale), ("pag_adaptive_scale", pag_adaptive_scale)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} = {v!r}: a finite number >= 0 (0 = off)")
    return float(pag_scale), float(pag_adaptive_scale)


def pag_scale_column(pag_scale: float, pag_adaptive_scale: float, timesteps) -> np.ndarray:
    """the PAG scale of every schedule entry, fp32 [n_ts] (diffusers' ``_get_pag_scale``): ``pag_scale`` itself without an
    adaptive scale, else max(pag_scale - pag_adaptive_scale * (1000 - t_i), 0); taken in float64, rounded once"""
    t = np.asarray(timesteps, dtype=np.float64)
    if pag_adaptive_scale == 0.0:
        return np.full(t.shape, pag_scale, dtype=np.float32)
    return np.maximum(pag_scale - pag_adaptive_scale * (1000.0 - t), 0.0).astype(np.float32)


def check_sag(sag_scale) -> float:
    """``sag_scale`` of diffusers' StableDiffusionSAGPipeline -> a float; negative or non-finite values (and booleans, which
    are no scales) are refused"""
    v = sag_scale
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0.0:
        raise ValueError(f"sag_scale = {v!r}: a finite number >= 0 (0 = off)")
    return float(v)


def refuse_sag_with(sag_scale: float, pag_scale: float = 0.0, guidance_rescale: float = 0.0, residuals: bool = False):
    """what self-attention guidance is not built together with (NotImplementedError before any launch)"""
    if sag_scale > 0.0 and pag_scale > 0.0:
        raise NotImplementedError("sag_scale > 0 together with pag_scale > 0 is not built: one of the two guidances per call")
    if sag_scale > 0.0 and guidance_rescale > 0.0:
        raise NotImplementedError("sag_scale > 0 together with guidance_rescale > 0 is not built (the rescale factor is defined "
                                  "on the classifier-free combine alone)")
    if sag_scale > 0.0 and residuals:
        raise NotImplementedError("SAG with ControlNet residuals is not built: pass sag_scale = 0 or run without a ControlNet "
                                  "/ precomputed residuals")


def check_eta(scheduler, eta: float, variance_noise=None) -> float:
    """``eta`` / ``variance_noise`` of the reference ``__call__``s (prepare_extra_step_kwargs -> DDIMScheduler.step(eta=,
    variance_noise=)): only DDIM has the term, its eta is in [0, 1], and the noise needs a coefficient -- which
    LCMScheduler's own noise has without eta (sqrt(1 - alphas_cumprod) of the next timestep).  -> float(eta)"""
    eta = float(eta)
    if eta == 0.0:
        if variance_noise is not None and not isinstance(scheduler, LCMScheduler):
            raise ValueError("variance_noise without eta: the noise term has the coefficient eta * sigma_t")
        return eta
    if not isinstance(scheduler, DDIMScheduler):
        raise ValueError(f"eta = {eta}: only DDIMScheduler has an eta term ({type(scheduler).__name__} is deterministic); "
                         "set pipe.scheduler = DDIMScheduler.from_config(pipe.scheduler.config) or pass eta = 0")
    if eta < 0.0:
        raise ValueError(f"eta = {eta}: DDIM's eta is in [0, 1]")
    return eta


# per schedule entry: the UNet's K/V rows [n_ts, 2B] int32, the ControlNets' [n_ts, B] int32 (or None), "merged" [n_ts] bool
StepRows = namedtuple("StepRows", "unet controlnet merged")


def step_rows(n_ts: int, first_step: int, start_merge_step: int, B: int, has_null_post: bool, device="cpu",
              controlnet: bool = True, single_pass: bool = False, pag: bool = False) -> StepRows:
    """The embed sets every schedule entry reads (ref :542-549: text-only while i <= start_merge_step, i counted from
    ``first_step`` like the reference's enumerate over the truncated timestep list).  The UNet's K/V cache holds rows
    [0,B) null, [B,2B) text-only, [2B,3B) augmented (ref :527-531) and, for SDXL's second unconditional set (ref SDXL
    :586-590, :620-631), [3B,4B) null-post: a step selects (null, text) before the merge, (null or null-post, augmented)
    after it.  A ControlNet's cache holds [0,B) text-only and [B,2B) augmented, selected the same way (CN :389-396).
    ``single_pass``: the UNet runs the conditional rows only -- [n_ts, B], text-only [B,2B) up to the merge and augmented
    [2B,3B) after it, in the same K/V row numbering.
    ``pag``: B more columns behind the others, the perturbed rows -- they read what the conditional rows read at every
    entry: [n_ts, 3B], or [n_ts, 2B] in the single pass."""
    ar = torch.arange(B, dtype=torch.int32, device=device)
    merged = torch.tensor([(i - first_step) > start_merge_step for i in range(n_ts)], device=device)
    pre = torch.cat([ar, ar + B])
    post = torch.cat([ar + (3 * B if has_null_post else 0), ar + 2 * B])
    cn = torch.where(merged[:, None], (ar + B)[None], ar[None]) if controlnet else None
    if single_pass:
        pre, post = ar + B, ar + 2 * B
    if pag:
        pre, post = torch.cat([pre, ar + B]), torch.cat([post, ar + 2 * B])
    return StepRows(torch.where(merged[:, None], post[None], pre[None]), cn, merged)


def captured_reads(unet, nets: Sequence[Any]) -> tuple:
    """What a captured step bakes in of the objects the engine does not own -- the UNet, then the ControlNets in the order
    they run -- as they are AFTER this generation's ``set_context`` calls: per object (its serial, its epoch, its
    ``context_addresses()``).  The serial tells two objects at the same addresses and shapes apart, and [A, B] from [B, A]; the
    epoch counts the changes of launch arguments kept on the host (``load_adapter_modules``: ip_scale) and the moves of the
    K/V buffers, so an address that went away and came back while another engine used the object is not taken for the old
    one.  A graph is valid only for the value it was captured under; nothing the step table carries (scales, merge step,
    ``first_step``) is in it."""
    return tuple((o.serial, o.epoch, tuple(o.context_addresses())) for o in (unet, *nets))


@dataclass
class _StepCoefficients:
    """The scheduler's side of a step: cid_cfg_ddim_step_f16 for the two first-order updates (DDIM at eta = 0, Euler),
    cid_cfg_multistep_step_f16 for PNDM, DPM-Solver++, DDIM with eta > 0 and LCM (history ring, remembered sample, noise
    row); cid_multistep_step_f16 for the single pass, whose ``eps`` is one model output per sample"""
    buf: torch.Tensor                           # the row the step table fills: 5 fp32, or the 16-word multistep row (cid.h)
    row: torch.Tensor                           # ``buf`` as the step kernel reads it (fp32)
    in_scale: torch.Tensor                      # the model-input scale inside ``row``: conv_in reads it in place
    table: torch.Tensor                         # [n_ts, ...] per-step rows, dtype of ``buf``
    hist: Optional[torch.Tensor] = None         # multistep: fp32 ring of earlier model outputs
    saved: Optional[torch.Tensor] = None        # multistep: the sample PNDM steps from twice
    z: Optional[torch.Tensor] = None            # DDIM eta > 0: the variance noise of every executed step; LCM: of all but the last
    escale: Optional[torch.Tensor] = None       # guidance_rescale: fp32 [B], the factor cid_cfg_rescale_f16 writes every step
    rescale: float = 0.0
    single_pass: bool = False
    pag: Optional[torch.Tensor] = None          # PAG: fp32 [1], this step's scale s_i (a step-table column)
    sag: float = 0.0                            # SAG: the scale, a launch argument of the +sag entries

    def update(self, eps, lat, guidance_scale, eps_d=None, **kw):
        if self.sag > 0.0:                      # eps_d: the prediction on the degraded latents, in a buffer of its own
            if self.single_pass:
                ops.sag_multistep_step(eps, lat, self.hist, self.saved, self.row, eps_d, self.sag, z=self.z, **kw)
            elif self.hist is None:
                ops.cfg_sag_ddim_step(eps, lat, self.buf, guidance_scale, eps_d, self.sag, **kw)
            else:
                ops.cfg_sag_multistep_step(eps, lat, self.hist, self.saved, self.row, guidance_scale, eps_d, self.sag,
                                           z=self.z, **kw)
            return
        if self.pag is not None:                # eps carries the perturbed rows behind the conditional ones
            if self.single_pass:
                ops.pag_multistep_step(eps, lat, self.hist, self.saved, self.row, self.pag, z=self.z, **kw)
            elif self.hist is None:
                ops.cfg_pag_ddim_step(eps, lat, self.buf, guidance_scale, self.pag, **kw)
            else:
                ops.cfg_pag_multistep_step(eps, lat, self.hist, self.saved, self.row, guidance_scale, self.pag, z=self.z, **kw)
            return
        if self.single_pass:                    # no CFG combine (and so no rescale of one)
            ops.multistep_step(eps, lat, self.hist, self.saved, self.row, z=self.z, **kw)
            return
        if self.escale is not None:             # UNet -> factor -> scaled step; the scaled entries of the same two kernels
            ops.cfg_rescale(eps, guidance_scale, self.rescale, self.escale, B=kw["B"], per_sample=kw["per_sample"])
            kw["escale"] = self.escale
        if self.hist is None:
            ops.cfg_ddim_step(eps, lat, self.buf, guidance_scale, **kw)
        else:
            ops.cfg_multistep_step(eps, lat, self.hist, self.saved, self.row, guidance_scale, z=self.z, **kw)


@dataclass
class _ControlPlan:
    """The ControlNets of one generation: a plain ``HipControlNet`` is a list of one whose scale is folded into its zero
    convs (``fold``; the UNet adds with cid_add_inplace_f16); a ``HipMultiControlNet`` runs unscaled and scale_k * keep_k[i]
    is a step-table column that cid_residual_accum_f16 reads (``scale_column``).  A column is (the static buffer the
    step's kernels read, the [n_ts, ...] table whose row i fills it) and is that buffer's only holder.  No net: all lists empty."""
    keep: List[List[float]]                     # [n_ts][nets]: the guidance windows (CN :363-370), 0 in skipped entries
    nets: list = field(default_factory=list)
    cond: List[torch.Tensor] = field(default_factory=list)      # per-net condition embedding
    kvrow: Optional[torch.Tensor] = None
    temb_column: Optional[tuple] = None         # (``cn_temb``, all nets' rows side by side): ONE table column (of 8)
    temb: List[Optional[torch.Tensor]] = field(default_factory=list)    # net k's slice of ``temb_column[0]`` (a view)
    fold: float = 1.0
    scale_column: Optional[tuple] = None        # multi only: (``cn_scale``, [n_ts, 4] scale_k * keep_k[i])


class DenoiseEngine:
    """The state that outlives a generation: the static buffers, the captured graphs and their warm-up keys"""

    def __init__(self, unet: HipUNet, scheduler: DDIMScheduler, use_graph: bool = True):
        self.unet = unet
        self.scheduler = scheduler
        self.use_graph = use_graph
        # captured step, keyed by the tuple of ControlNets that run in it (() = none); valid while no static buffer moved
        # and the configuration key (which holds captured_reads) is the same: invalidate()
        self._graphs: Dict[Any, Any] = {}
        self._warm_keys = set()
        self._config_key = None
        self.captures: List[Any] = []           # key of every capture this engine ever made, in order (re-captures show twice)
        self._static: Dict[str, torch.Tensor] = {}
        # the step launch of the last run: "cfg_ddim" or "cfg_multistep", "+rescale" with guidance_rescale; "multistep" = the
        # single pass; "+pag" with perturbed-attention guidance ("cfg_ddim+pag", "cfg_multistep+pag", "multistep+pag"), "+sag"
        # with self-attention guidance
        self.step_path: Optional[str] = None

    @property
    def sag_mass(self) -> Optional[torch.Tensor]:
        """fp32 [B, H_mid * W_mid]: the column mass the last evaluation of a run with ``sag_scale`` > 0 thresholded"""
        return self._static.get("sag_mass")

    def invalidate(self):
        """forget the captured graphs AND their eager warm-up (the first step after a change must run eagerly again)"""
        self._graphs.clear()
        self._warm_keys.clear()

    def _launch(self, step, key):
        """``step(key)``: eager without graphs and the first time a key occurs, captured the second time, replayed from then on"""
        if not self.use_graph:
            step(key)
        elif key not in self._warm_keys:
            step(key)   # eager warm-up: configures kernels, sizes the allocator pools
            self._warm_keys.add(key)
        else:
            g = self._graphs.get(key)
            if g is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    step(key)
                self._graphs[key] = g
                self.captures.append(key)
            g.replay()

    def _static_tensor(self, name: str, like: torch.Tensor, dtype=None) -> torch.Tensor:
        """persistent device buffer (stable address across generations -> the captured graph stays valid)"""
        dtype = dtype or like.dtype
        cur = self._static.get(name)
        if cur is None or cur.shape != like.shape or cur.dtype != dtype:
            cur = torch.empty(like.shape, dtype=dtype, device=self.unet.device)
            self._static[name] = cur
            self.invalidate()   # an address changed: re-capture
        cur.copy_(like.to(device=self.unet.device, dtype=dtype))
        return cur

    def _step_coefficients(self, lat, inpaint: bool, first_step: int, eta: float, variance_noise,
                           single_pass: bool = False) -> _StepCoefficients:
        sch, S, dev = self.scheduler, self._static_tensor, self.unet.device
        n_ts = len(sch.timesteps)
        multistep = bool(getattr(sch, "multistep", False)) or eta > 0.0
        self.step_path = "multistep" if single_pass else "cfg_multistep" if multistep else "cfg_ddim"
        if not multistep:
            table = torch.from_numpy(sch.coefficient_table(inpaint)).to(dev).view(n_ts, 5).float()
            buf = S("coef", torch.zeros(5), torch.float32)      # c_x, c_eps, c_init, c_noise, model-input scale
            return _StepCoefficients(buf, buf, buf[4:5], table)
        rows = sch.coefficient_rows(inpaint, first_step, np.float32, **({"eta": eta} if eta > 0.0 else {}))
        table = torch.from_numpy(pack_step_rows(rows)).to(dev).view(n_ts, 16)
        z = None
        if eta > 0.0:
            n_run = n_ts - first_step
            if variance_noise is None or tuple(variance_noise.shape) != (n_run, *lat.shape):
                raise ValueError(f"eta = {eta} needs variance_noise of shape {(n_run, *lat.shape)} (one tensor per executed "
                                 f"step), got {None if variance_noise is None else tuple(variance_noise.shape)}")
            z = S("z", variance_noise, torch.float16)
        elif isinstance(sch, LCMScheduler) and n_ts - first_step > 1:
            n_z = n_ts - first_step - 1
            if variance_noise is None or tuple(variance_noise.shape) != (n_z, *lat.shape):
                raise ValueError(f"LCMScheduler over {n_z + 1} executed steps needs variance_noise of shape {(n_z, *lat.shape)} "
                                 f"(one tensor per executed step but the last), got "
                                 f"{None if variance_noise is None else tuple(variance_noise.shape)}")
            z = S("z", variance_noise, torch.float16)
        buf = S("ms_row", torch.zeros(16), torch.int32)     # the multistep row (cid.h): 12 fp32 words, 4 int32 words
        row = buf.view(torch.float32)
        return _StepCoefficients(buf, row, row[C_IN:C_IN + 1], table,
                                 hist=S("ms_hist", torch.zeros(4, lat.numel()), torch.float32),
                                 saved=S("ms_saved", torch.zeros(lat.numel()), torch.float16), z=z, single_pass=single_pass)

    def _control_plan(self, controlnet, control_image, conditioning_scale, starts, ends, text_embeds, augmented_embeds,
                      rows: StepRows, tvals, first_step: int, temb_table: bool) -> _ControlPlan:
        """native ControlNets (CN :389-412; MultiControlNet CN :281-301, :363-370, :397-398): conditional latents +
        conditional embeds, residuals recomputed per step.  Every net has its own context, condition embedding and keep
        window; they share the embed-row selector."""
        S, dev, n_ts = self._static_tensor, self.unet.device, len(tvals)
        if controlnet is None:
            return _ControlPlan(keep=[[]] * n_ts)
        multi = isinstance(controlnet, HipMultiControlNet)
        if not multi:       # a plain net is a list of one
            control_image, starts, ends = [control_image], [starts], [ends]
        plan = _ControlPlan(keep=controlnet_keep_table(n_ts - first_step, starts, ends, first_step),
                            nets=controlnet.nets if multi else [controlnet])
        ehs = torch.cat([text_embeds.to(dev), augmented_embeds.to(dev)], dim=0)
        for net in plan.nets:
            net.set_context(ehs, num_tokens=0)
        plan.cond = [S(f"cn_cond{k}", net.cond_embedding(img), torch.float16) for k, (net, img) in
                     enumerate(zip(plan.nets, control_image))]
        plan.kvrow = S("cn_kvrow", rows.controlnet[0], torch.int32)
        plan.temb = [None] * len(plan.nets)
        if temb_table:
            tabs = [net.time_embed_table(tvals) for net in plan.nets]
            assert all(t.shape[1] % 8 == 0 for t in tabs), "time-embedding rows are 16-byte multiples"
            tab = torch.cat(tabs, dim=1) if len(tabs) > 1 else tabs[0]
            plan.temb_column = (S("cn_temb", tab[:1], torch.float16), tab.view(n_ts, -1))
            plan.temb = list(plan.temb_column[0].split([t.shape[1] for t in tabs], dim=1))
        if multi:
            # the zero convs stay unscaled: a new scale needs no new weights or graph
            tab = torch.zeros(n_ts, 4)
            tab[:, :len(plan.nets)] = torch.tensor(plan.keep, dtype=torch.float64).mul(
                torch.tensor(list(conditioning_scale), dtype=torch.float64)).float()
            plan.scale_column = (S("cn_scale", torch.zeros(4), torch.float32), tab.to(dev))    # 4 fp32 = one 16-byte column
        else:
            plan.fold = float(conditioning_scale)
        return plan

    @torch.no_grad()
    def run(self, latents: torch.Tensor, null_embeds, augmented_embeds, text_embeds, *, num_inference_steps: int,
            guidance_scale: float, start_merge_step: int, null_embeds_post=None, first_step: int = 0,
            pooled: Optional[Sequence[torch.Tensor]] = None, time_ids: Optional[torch.Tensor] = None,
            down_residuals=None, mid_residual=None, inpaint_mask=None, inpaint_init=None, inpaint_noise=None,
            controlnet=None, control_image=None, conditioning_scale: Union[float, Sequence[float]] = 1.0,
            control_guidance_start: Union[float, Sequence[float]] = 0.0,
            control_guidance_end: Union[float, Sequence[float]] = 1.0,
            callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: int = 1,
            scale_initial: bool = True, unet_extra: Optional[torch.Tensor] = None, eta: float = 0.0,
            variance_noise: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0, pag_scale: float = 0.0,
            pag_adaptive_scale: float = 0.0, sag_scale: float = 0.0):
        """``sag_scale`` > 0: self-attention guidance.  The guide rows -- the unconditional ones, the
        conditional ones in the single pass -- give the column mass of the mid block's first self-attention map; where it
        exceeds 1 their predicted sample is blurred, the result is noised again with their predicted noise, and a second
        UNet evaluation of those B rows on it (same context rows, time row, SDXL conditioning and ``unet_extra``) gives e_d:
        e = u + g (c - u) + s (u - e_d), e = c + s (c - e_d) in the single pass.  Refused (NotImplementedError) together with
        ``pag_scale`` > 0, ``guidance_rescale`` > 0 and a ControlNet or ControlNet residuals.  At 0 nothing changes.
        ``pag_scale`` > 0: perturbed-attention guidance.  The UNet runs B more batch rows, the
        perturbed evaluation of the conditional rows (same latents, time row, context rows and SDXL conditioning; identity
        self-attention in the layers ``unet.enable_pag`` selected, the default ``("mid",)`` if none were), and the step is
        e = u + g (c - u) + s_i (c - p) -- e = c + s_i (c - p) in the single pass -- with s_i = ``pag_scale``, or
        max(pag_scale - ``pag_adaptive_scale`` * (1000 - t_i), 0), a step-table column.  Refused (NotImplementedError)
        together with ``guidance_rescale`` > 0 and with a ControlNet or ControlNet residuals.  At 0 nothing changes.
        ``guidance_rescale`` > 0 with ``guidance_scale`` > 1 (diffusers' condition): every step runs UNet ->
        cid_cfg_rescale_f16 (the per-sample factor, into a static buffer) -> the scaled step entry; at 0 the step is the
        one it always was.
        Under ``LCMScheduler`` ``guidance_scale`` <= 1 takes the single pass (module docstring): the UNet runs the B
        conditional rows and ``guidance_rescale`` is inert, as it is at ``guidance_scale`` <= 1 everywhere.  A UNet with
        ``time_cond_proj_dim`` takes it at every ``guidance_scale`` (the scale conditions its time embedding), needs
        LCMScheduler and refuses ``guidance_rescale`` > 0.  LCM's noise comes as ``variance_noise`` [executed steps - 1, B, C, h, w].
        ``eta`` > 0 (DDIMScheduler only) with ``variance_noise`` [executed steps, B, C, h, w]: the noise diffusers' DDIM
        ``step(..., eta=, variance_noise=)`` adds, one tensor per executed step in loop order.
        ``first_step``: the loop runs schedule entries [first_step, S) -- the inpaint pipelines' ``strength`` < 1
        window (get_timesteps, inpaint ref :246-252); the embed switch and the ControlNet keep window count steps from
        there, exactly like the reference's ``for i, t in enumerate(timesteps)`` over the truncated list.
        ``unet_extra`` [B, 5, h, w]: cat([mask, masked_image_latents]) of a 9-channel inpainting UNet (inpaint ref
        :320-321, CN :415-416) -- conv_in reads it beside the (scaled) latents, the ControlNet does not see it.
        ``controlnet`` = a ``HipMultiControlNet``: ``control_image``, ``conditioning_scale``, ``control_guidance_start`` and
        ``control_guidance_end`` are sequences with one entry per net."""
        unet, sch, S = self.unet, self.scheduler, self._static_tensor
        eta = check_eta(sch, eta, variance_noise)
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        pag_scale, pag_adaptive_scale = check_pag(pag_scale, pag_adaptive_scale)
        pag = pag_scale > 0.0
        sag_scale = check_sag(sag_scale)
        refuse_sag_with(sag_scale, pag_scale, guidance_rescale,
                        controlnet is not None or down_residuals is not None or mid_residual is not None)
        if pag and guidance_rescale > 0.0:
            raise NotImplementedError("pag_scale > 0 together with guidance_rescale > 0 is not built (the rescale factor is "
                                      "defined on the classifier-free combine alone)")
        if pag and (controlnet is not None or down_residuals is not None or mid_residual is not None):
            raise NotImplementedError("PAG with ControlNet residuals is not built: pass pag_scale = 0 or run without a "
                                      "ControlNet / precomputed residuals")
        if pag and not unet.pag_layers:
            unet.enable_pag()                   # diffusers' default pag_applied_layers
        dev, B = unet.device, latents.shape[0]
        lcm = isinstance(sch, LCMScheduler)
        embedded_guidance = getattr(unet.config, "time_cond_proj_dim", None) is not None
        if embedded_guidance and not lcm:
            raise NotImplementedError(f"{type(sch).__name__} on a UNet with time_cond_proj_dim: a distilled latent consistency "
                                      "model is sampled with LCMScheduler (pipe.scheduler = LCMScheduler.from_config("
                                      "pipe.scheduler.config))")
        if embedded_guidance and guidance_rescale > 0.0:
            raise ValueError(f"guidance_rescale = {guidance_rescale}: a UNet with time_cond_proj_dim takes guidance_scale in its "
                             "time embedding; there is no classifier-free combine to rescale")
        single = lcm and (embedded_guidance or guidance_scale <= 1.0)
        n_b = (B if single else 2 * B) + (B if pag else 0)      # the UNet's batch rows: [uncond |] cond [| perturbed]
        sch.set_timesteps(num_inference_steps)                      # ref :510, before prepare_latents (:517)
        # prepare_latents (diffusers; ref :517-526) scales the initial noise by the scheduler's init_noise_sigma
        lat = S("lat", latents.to(dev).float() * (float(sch.init_noise_sigma) if scale_initial else 1.0), torch.float16)
        # rows [0,B) null, [B,2B) text-only, [2B,3B) augmented   (ref :527-531 + :542-549); the SDXL pipeline has a
        # second unconditional set for the steps after the merge (ref SDXL :586-590, :620-631): rows [3B,4B)
        sets = [null_embeds.to(dev), text_embeds.to(dev), augmented_embeds.to(dev)]
        if null_embeds_post is not None:
            sets.append(null_embeds_post.to(dev))
        unet.set_context(torch.cat(sets, dim=0))
        ts = sch.timesteps
        n_ts = len(ts)
        inpaint = inpaint_mask is not None
        coef = self._step_coefficients(lat, inpaint, first_step, eta, variance_noise, single)
        if guidance_rescale > 0.0 and guidance_scale > 1.0 and not single:
            coef.escale, coef.rescale = S("escale", torch.ones(B), torch.float32), guidance_rescale
            self.step_path += "+rescale"
        pag_column = None
        if pag:
            coef.pag = S("pag", torch.zeros(1), torch.float32)
            pag_column = (coef.pag, torch.from_numpy(pag_scale_column(pag_scale, pag_adaptive_scale, sch.timesteps)).view(-1, 1))
            self.step_path += "+pag"
        sag_column = None
        if sag_scale > 0.0:
            coef.sag = sag_scale
            sag_coef = S("sag_coef", torch.zeros(8), torch.float32)
            sag_column = (sag_coef, torch.from_numpy(sag_coefficient_table(sch)).to(dev))
            hm, wm = unet.mid_size(lat.shape[2], lat.shape[3])
            sag_mass = S("sag_mass", torch.zeros(B, hm * wm), torch.float32)
            sag_xdeg = S("sag_xdeg", torch.zeros_like(lat), torch.float16)
            self.step_path += "+sag"
        tvals = torch.tensor(ts.astype(np.float32), device=dev)
        rows = step_rows(n_ts, first_step, start_merge_step, B, null_embeds_post is not None, dev, controlnet is not None,
                         single_pass=single, pag=pag)
        t_buf = S("t", torch.zeros(1), torch.float32)
        kvrow = S("kvrow", rows.unet[0], torch.int32)
        added = None
        if time_ids is not None:
            p_null, p_text, p_aug = [p.to(device=dev, dtype=torch.float16) for p in pooled]
            def stack(neg, pos):
                """the UNet's batch rows of a per-row condition: [neg |] pos [| pos] -- no unconditional rows in the single
                pass, and with PAG the perturbed rows repeat the conditional rows' values"""
                return torch.cat(([] if single else [neg]) + [pos] * (2 if pag else 1), 0)
            # time_ids is [2B, 6], negative rows first: the last B rows are the conditional ones (without PAG the two slices
            # put together again are the tensor as it came, whatever its row count; the single pass keeps its last B rows)
            tid = time_ids.to(dev)
            added = {"text_embeds": S("pooled", stack(p_null, p_text), torch.float16),
                     "time_ids": S("time_ids", stack(tid[:-B], tid[-B:]), torch.float32)}
        blend = dict(mask=None, init=None, noise=None)
        if inpaint:
            if unet_extra is not None:
                raise ValueError("a 9-channel inpainting UNet is not blended: the reference guards the mask blend with "
                                 "`if num_channels_unet == 4` (inpaint ref :340, CN :437)")
            if inpaint_init is None or inpaint_noise is None:
                raise ValueError("the mask blend of a 4-channel UNet needs image_latents and noise (inpaint ref :340-353)")
            blend = dict(mask=S("mask", inpaint_mask.to(dev).expand_as(lat), torch.float16),
                         init=S("init", inpaint_init, torch.float16), noise=S("noise", inpaint_noise, torch.float16))
        extra = S("unet_extra", unet_extra, torch.float16) if unet_extra is not None else None
        dres = mres = None
        if down_residuals is not None:
            assert controlnet is None, "pass either a ControlNet or precomputed residuals"
            dres = [S(f"dres{j}", r, torch.float16) for j, r in enumerate(down_residuals)]
            mres = S("mres", mid_residual, torch.float16)
        # time path: one table per generation instead of three weight-streaming GEMVs per step (not with SDXL's
        # text_time conditioning, whose rows also depend on the sample)
        temb_tab = temb_buf = None
        if unet.config.addition_embed_type is None and not os.environ.get("CID_NO_TEMB_TABLE"):
            # (with time_cond_proj_dim the rows also depend on guidance_scale: built anew in every generation, like this)
            temb_tab = unet.time_embed_table(tvals, **({"guidance_scale": guidance_scale} if embedded_guidance else {}))
            temb_buf = S("temb", temb_tab[:1], torch.float16)
        elif embedded_guidance:
            unet.set_guidance_embedding(guidance_scale)     # the per-step time path adds this row (a buffer at a stable address)
        cn =self._control_plan(controlnet, control_image, conditioning_scale, control_guidance_start, control_guidance_end,
                                text_embeds, augmented_embeds, rows, tvals, first_step, temb_buf is not None)
        # every per-step host value of the reference's `for i, t in enumerate(timesteps)` as one device table: row i holds t,
        # the scheduler coefficients, the embed-set rows, the time-embedding row and SDXL's pooled embeds (ref SDXL
        # :620-631); cid_step_select, the first launch of the captured step, copies row `counter` into the buffers the
        # step's kernels read and increments the counter
        cols = [(t_buf, tvals.view(n_ts, 1)), (coef.buf, coef.table), (kvrow, rows.unet)]
        if cn.nets:
            cols.append((cn.kvrow, rows.controlnet))
        if temb_buf is not None:
            cols.append((temb_buf, temb_tab.view(n_ts, -1)))
        cols += [c for c in (cn.temb_column, cn.scale_column, pag_column, sag_column) if c is not None]
        if added is not None:
            pre, post = stack(p_null, p_text), stack(p_null, p_aug)
            cols.append((added["text_embeds"], torch.where(rows.merged[:, None, None], post[None], pre[None])))
        table = ops.StepTable(cols, dev, alloc=S)     # table + counter are static buffers too
        table.reset(first_step)

        # every static buffer exists now (a new one has invalidated the graphs); so does a new configuration, and so does
        # anything else than what the graphs were captured under in the UNet or the nets (another object, moved K/V or
        # workspace, a new epoch) -- whoever changed it, this engine or another one that shares the object.  The multi path
        # reads its scales from the step table: they are not part of the key
        unet.reserve_workspace(n_b)
        for net in cn.nets:
            net.reserve_workspace(B)
        key = (captured_reads(unet, cn.nets), B, tuple(lat.shape), float(guidance_scale), inpaint, time_ids is not None,
               dres is not None, bool(cn.nets), ("multi", len(cn.nets)) if cn.scale_column else cn.fold, extra is not None,
               coef.hist is not None, coef.z is not None, coef.rescale, single, pag, n_b, coef.sag)
        if key != self._config_key:
            self.invalidate()
            self._config_key = key
        per_sample = lat[0].numel()
        if coef.sag > 0.0:
            # every forward hands its buffers out anew: the second one would reuse the first one's output, so that is kept here
            sag_eps = S("sag_eps", torch.zeros(n_b, unet.config.out_channels, *lat.shape[2:]), torch.float16)
            # the guide rows lead the batch in both forms, and so do their context rows and SDXL conditions
            added_g = None if added is None else {k: v[:B] for k, v in added.items()}

        def sag_step():
            """select -> UNet(n_b), with the guide rows' column mass -> degrade -> UNet(B) on the degraded latents -> step"""
            eps = unet.forward_tokens(lat, t_buf, kvrow, n_b, added, temb=temb_buf, in_scale=coef.in_scale, extra=extra,
                                      sag=(sag_mass, 0, B))
            sag_eps.copy_(eps)
            ops.sag_degrade(lat, sag_eps[:B], sag_mass, sag_xdeg, sag_coef, hm=hm, wm=wm)
            eps_d = unet.forward_tokens(sag_xdeg, t_buf, kvrow[:B], B, added_g, temb=temb_buf, in_scale=coef.in_scale,
                                        extra=extra)
            coef.update(sag_eps, lat, guidance_scale, eps_d=eps_d, B=B, per_sample=per_sample, **blend)

        def step(active):
            """``active``: the nets that run, () = none -- one forward after another on the current stream (no forked
            capture streams, no parallel graph branches)"""
            table.select()
            if coef.sag > 0.0:                  # (no ControlNet, no residuals: refused above)
                return sag_step()
            d, m, scales = dres, mres, None
            res = {k: cn.nets[k].forward_tokens(lat, t_buf, cn.kvrow, B, cn.cond[k], cn.fold, temb=cn.temb[k],
                                                in_scale=coef.in_scale) for k in active}
            if res and cn.scale_column is None:
                d, m = res[0]               # scale folded into the zero convs: the UNet adds the residuals as they are
            elif res:
                # unscaled residuals (None: the net did not run); the UNet adds sum_k cn_scale[k] * r_k in two launches
                d, m = ([res[k][j] if k in res else None for k in range(len(cn.nets))] for j in (0, 1))
                scales = cn.scale_column[0]
            eps = unet.forward_tokens(lat, t_buf, kvrow, n_b, added, d, m, temb=temb_buf, in_scale=coef.in_scale,
                                      extra=extra, residual_scales=scales, pag_rows=B if pag else 0)
            coef.update(eps, lat, guidance_scale, B=B, per_sample=per_sample, **blend)

        for i in range(first_step, n_ts):
            active = active_nets(cn.keep[i])     # only nets with keep > 0 run (CN :397-403); their tuple keys warm-up and graph
            self._launch(step, active)
            if callback is not None and (i - first_step) % callback_steps == 0:
                callback(i - first_step, int(ts[i]), lat)
        return lat.clone()
