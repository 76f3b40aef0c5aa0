"""state_dict (diffusers names) + ``adapter_modules`` -> device-resident fp16 weights in
the layouts the HIP kernels consume.

Done once at load time (the reference's UNet and adapters are frozen at inference):
  * LoRA merge  W' = W + lora_scale * up @ down   (attention.py:139,146,147,162 / :236,249,250,282)
  * softmax scale d^-0.5 (diffusers Attention.scale) and log2(e) folded into W'_q
  * self-attn q/k/v concatenated to one [3C, C] matrix (one GEMM launch pair)
  * cross-attn text and ID key/value projections concatenated to [2C, Dc] each
  * 3x3 conv weights [Cout, Cin, 3, 3] -> [Cout, 9, Cin] (tap-major, channel-contiguous K axis)
  * GEGLU projection rows interleaved in blocks of 16 (value block, gate block)
  * all ResnetBlock2D.time_emb_proj stacked into one [sum(Cout), 4*C0] matrix
  * cross-attn Wq'/Wo' stay row-major [C, C]: the fused kernel streams 32-deep slabs of them by DMA
All arithmetic for the merge is fp32 on the target device, rounded once to fp16.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import ops
from .lora import merged_delta
from .unet_spec import UNetConfig, attn_processor_names, walk

LOG2E = 1.4426950408889634


def _h(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.float16).contiguous()


def _f(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.float32)


def _conv3(w: torch.Tensor, dev) -> torch.Tensor:
    co, ci, kh, kw = w.shape
    return _h(w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci), dev)


GEGLU_BLOCK = 16   # one MFMA tile of output channels


def _geglu_interleave(t: torch.Tensor) -> torch.Tensor:
    """rows [value(4C) | gate(4C)] -> blocks of 16: v0 g0 v1 g1 ... (a lane of the GEMM then holds
    a value and its gate in the same accumulator slot of two adjacent tiles)"""
    n2 = t.shape[0]
    half = n2 // 2
    v = t[:half].reshape(half // GEGLU_BLOCK, GEGLU_BLOCK, *t.shape[1:])
    g = t[half:].reshape(half // GEGLU_BLOCK, GEGLU_BLOCK, *t.shape[1:])
    return torch.stack([v, g], dim=1).reshape(n2, *t.shape[1:])


def fold_ff2_proj_out(w2: torch.Tensor, b2: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor):
    """ff2 and proj_out of a transformer's tail as one linear map over the row [ff | h3] (nothing non-linear lies between:
    out = Wp (W2 ff + b2 + h3) + bp + x):  W' = [Wp W2 | Wp]  [c, 5c],  b' = Wp b2 + bp.  The operands are the fp16-rounded
    tensors the two-launch path uses; the products are taken in fp64 and rounded to fp16 once."""
    wp64, w264 = wp.half().double(), w2.half().double()
    w = torch.cat([wp64 @ w264, wp64], 1).half().contiguous()
    b = (wp64 @ b2.half().double() + bp.half().double()).half().contiguous()
    return w, b


def fold_ln(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """LayerNorm in front of a projection, folded (cid_gemm_desc.ln_s / ln_b):  LN(x) W^T + bias =
    rstd * (x W'^T - mean * s) + b'  with  W' = W diag(gamma) rounded to fp16, s = row sums of the ROUNDED W' (the mean
    term then cancels exactly), b' = W beta + bias.  ``w`` fp32 [N, C].  Returns (W' fp16, s, b') with the two fp32 vectors
    stored as raw bits in fp16-typed tensors (the broadcast arena is one dtype; use ``.view(torch.float32)``)."""
    w = w.float()
    wf = (w * gamma.float()[None, :]).half().contiguous()
    s = wf.float().sum(1).contiguous()
    b = w @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return wf, s.view(torch.float16), b.contiguous().view(torch.float16)


def fold_vo(wv: torch.Tensor, wo: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
            bias: Optional[torch.Tensor] = None):
    """Identity self-attention (perturbed-attention guidance): without the attention map ``to_out(to_v(LN(x)))`` is ONE
    linear map.  ``wv``, ``wo`` fp32 [C, C] (merged) -> Wvo = Wo Wv, the product taken in fp32 on the operands' device, then
    norm1 folded exactly as :func:`fold_ln` does: returns (W' = Wvo diag(gamma) fp16, s, b') for ``ops.gemm(..., ln=)`` --
    s the row sums of the ROUNDED W', b' = Wvo beta + ``bias`` (to_out's bias, which the folded launch cannot take apart),
    both fp32 as raw bits in fp16-typed tensors.  One rounding to fp16 of the composed weight, where the two-GEMM path rounds
    Wv, the intermediate activation and Wo."""
    return fold_ln(wo.float() @ wv.float(), gamma, beta, bias)


PAG_SUFFIXES = ("w", "wl", "lns", "lnb")     # per selected block: attn1.vo.{w: Wvo fp16 (LayerNorm launch + GEMM), wl / lns / lnb: fold_vo}


class PackedUNet:
    """Holds every packed tensor; ``w[name]`` lookups use diffusers-style prefixes."""

    def __init__(self, cfg: UNetConfig, unet_sd: Dict[str, torch.Tensor],
                 adapter_sd: Optional[Dict[str, torch.Tensor]], device, lora_scale: float = 1.0,
                 encoder_only: bool = False, keep_base: bool = False):
        """``keep_base``: keep the un-merged attention projection weights (fp16, ~10 % of the model) so that
        ``load_adapter_modules`` can merge a ConsistentID checkpoint's LoRA / ID projections later, in place -- and, on the
        HOST, references to the source tensors of the other LoRA-able weights (``ff.net.0.proj``, ``ff.net.2``, ``proj_in``,
        ``proj_out``) for ``set_lora``: no device memory, but the state dict's tensors stay alive.
        ``encoder_only``: ``unet_sd`` is a diffusers ControlNetModel state_dict -- the UNet's encoder half plus
        ``controlnet_cond_embedding.*`` / ``controlnet_down_blocks.*`` / ``controlnet_mid_block.*``."""
        self.cfg = cfg
        self.encoder_only = encoder_only
        self._base_attn: Dict[str, torch.Tensor] = {}
        self._base_host: Dict[str, torch.Tensor] = {}       # ff / proj_in / proj_out sources for set_lora (host tensors)
        self._lora: list = []                               # active (modules, weight) entries of set_lora
        self._lora_scale = lora_scale
        self._adapter_sd, self._adapter_scale = (adapter_sd, lora_scale) if keep_base else (None, lora_scale)
        self.device = device
        self.w: Dict[str, torch.Tensor] = {}
        self.temb_offsets: Dict[str, int] = {}
        self.ip_scale: Dict[str, float] = {}
        # perturbed-attention guidance (set_pag): the folded to_out . to_v weights of the selected blocks only, BESIDE ``w`` --
        # an engine that never enables PAG holds the keys and the bytes it always held
        self.pag: Dict[str, torch.Tensor] = {}
        self._pag_blocks: tuple = ()
        dev = device
        sd = unet_sd
        W = self.w
        downs, mid, ups = walk(cfg)
        if encoder_only:
            ups = []
        proc_index = {n: i for i, n in enumerate(attn_processor_names(cfg))}

        # ---- ends + time path
        W["conv_in.w"] = _h(sd["conv_in.weight"].permute(0, 2, 3, 1).reshape(sd["conv_in.weight"].shape[0], -1), dev)
        W["conv_in.b"] = _h(sd["conv_in.bias"], dev)
        if not encoder_only:
            W["conv_out.w"] = _h(sd["conv_out.weight"].permute(0, 2, 3, 1).reshape(sd["conv_out.weight"].shape[0], -1), dev)
            W["conv_out.b"] = _h(sd["conv_out.bias"], dev)
            for n in ("conv_norm_out",):
                W[f"{n}.g"], W[f"{n}.b"] = _h(sd[f"{n}.weight"], dev), _h(sd[f"{n}.bias"], dev)
        else:
            # condition embedding: (name, cin, cout, stride, silu) in execution order; zero convs as [C, C] matrices
            self.cond_convs = []
            e = "controlnet_cond_embedding"
            names = [f"{e}.conv_in"]
            i = 0
            while f"{e}.blocks.{i}.weight" in sd:
                names.append(f"{e}.blocks.{i}")
                i += 1
            names.append(f"{e}.conv_out")
            for n in names:
                w = sd[f"{n}.weight"]
                stride = 2 if (n.startswith(f"{e}.blocks.") and int(n.rsplit(".", 1)[1]) % 2 == 1) else 1
                W[f"{n}.w"], W[f"{n}.b"] = _conv3(w, dev), _h(sd[f"{n}.bias"], dev)
                self.cond_convs.append((n, w.shape[1], w.shape[0], stride, n != f"{e}.conv_out"))
            self.n_zero = 0
            while f"controlnet_down_blocks.{self.n_zero}.weight" in sd:
                n = f"controlnet_down_blocks.{self.n_zero}"
                c = sd[f"{n}.weight"].shape[0]
                W[f"{n}.w"], W[f"{n}.b"] = _h(sd[f"{n}.weight"].reshape(c, c), dev), _h(sd[f"{n}.bias"], dev)
                self.n_zero += 1
            c = sd["controlnet_mid_block.weight"].shape[0]
            W["controlnet_mid_block.w"] = _h(sd["controlnet_mid_block.weight"].reshape(c, c), dev)
            W["controlnet_mid_block.b"] = _h(sd["controlnet_mid_block.bias"], dev)
        for n in ("time_embedding.linear_1", "time_embedding.linear_2") + (
                ("add_embedding.linear_1", "add_embedding.linear_2") if cfg.addition_embed_type else ()):
            W[f"{n}.w"], W[f"{n}.b"] = _h(sd[f"{n}.weight"], dev), _h(sd[f"{n}.bias"], dev)
        if cfg.time_cond_proj_dim is not None:      # [c0, dim], no bias: the guidance-scale embedding of a distilled LCM
            if cfg.time_cond_proj_dim % 8:
                raise NotImplementedError(f"time_cond_proj_dim = {cfg.time_cond_proj_dim}: a multiple of 8 (cid_linear_small_f16)")
            W["time_embedding.cond_proj.w"] = _h(sd["time_embedding.cond_proj.weight"], dev)

        # ---- resnets (+ stacked time_emb_proj)
        tw, tb, off = [], [], 0
        for blk in downs + [mid] + ups:
            for r in blk.resnets:
                n = r.name
                W[f"{n}.norm1.g"], W[f"{n}.norm1.b"] = _h(sd[f"{n}.norm1.weight"], dev), _h(sd[f"{n}.norm1.bias"], dev)
                W[f"{n}.norm2.g"], W[f"{n}.norm2.b"] = _h(sd[f"{n}.norm2.weight"], dev), _h(sd[f"{n}.norm2.bias"], dev)
                W[f"{n}.conv1.w"], W[f"{n}.conv1.b"] = _conv3(sd[f"{n}.conv1.weight"], dev), _h(sd[f"{n}.conv1.bias"], dev)
                W[f"{n}.conv2.w"], W[f"{n}.conv2.b"] = _conv3(sd[f"{n}.conv2.weight"], dev), _h(sd[f"{n}.conv2.bias"], dev)
                if r.cin != r.cout:
                    W[f"{n}.short.w"] = _h(sd[f"{n}.conv_shortcut.weight"].reshape(r.cout, r.cin), dev)
                    W[f"{n}.short.b"] = _h(sd[f"{n}.conv_shortcut.bias"], dev)
                tw.append(sd[f"{n}.time_emb_proj.weight"]); tb.append(sd[f"{n}.time_emb_proj.bias"])
                self.temb_offsets[n] = off
                off += r.cout
            if blk.sampler:
                n = f"{blk.name}.{blk.sampler}.conv"
                W[f"{n}.w"], W[f"{n}.b"] = _conv3(sd[f"{n}.weight"], dev), _h(sd[f"{n}.bias"], dev)
                if blk.sampler.startswith("upsamplers") and W[f"{n}.w"].is_cuda:
                    # Upsample2D: the nine taps folded into four 2x2 phase convolutions (ops.gemm w_up4), once per load
                    W[f"{n}.w4"] = ops.upconv_fold(W[f"{n}.w"])
        self.temb_total = off
        W["temb_all.w"] = _h(torch.cat([t.to(torch.float32) for t in tw], 0), dev)
        W["temb_all.b"] = _h(torch.cat([t.to(torch.float32) for t in tb], 0), dev)

        # ---- transformers
        self.xattn_layers: List[str] = []
        for blk in downs + [mid] + ups:
            for t in blk.attentions:
                n, c = t.name, t.channels
                d = c // t.heads
                W[f"{n}.norm.g"], W[f"{n}.norm.b"] = _h(sd[f"{n}.norm.weight"], dev), _h(sd[f"{n}.norm.bias"], dev)
                for p in ("proj_in", "proj_out"):
                    W[f"{n}.{p}.w"] = _h(sd[f"{n}.{p}.weight"].reshape(c, c), dev)
                    W[f"{n}.{p}.b"] = _h(sd[f"{n}.{p}.bias"], dev)
                for k in range(t.n_layers):
                    b = f"{n}.transformer_blocks.{k}"
                    for ln in ("norm1", "norm2", "norm3"):
                        W[f"{b}.{ln}.g"], W[f"{b}.{ln}.b"] = _h(sd[f"{b}.{ln}.weight"], dev), _h(sd[f"{b}.{ln}.bias"], dev)
                    for k_, v_ in self._attention_weights(b, d, sd, adapter_sd, proc_index, lora_scale,
                                                          ln2=(W[f"{b}.norm2.g"], W[f"{b}.norm2.b"]),
                                                          ln1=(W[f"{b}.norm1.g"], W[f"{b}.norm1.b"])).items():
                        W[k_] = v_
                    W[f"{b}.attn1.out.b"] = _h(sd[f"{b}.attn1.to_out.0.bias"], dev)
                    W[f"{b}.attn2.bo"] = _h(sd[f"{b}.attn2.to_out.0.bias"], dev)
                    self.ip_scale[b] = 1.0 if adapter_sd is not None else 0.0
                    if keep_base:
                        for a in ("attn1", "attn2"):
                            for w_ in ("to_q", "to_k", "to_v", "to_out.0"):
                                self._base_attn[f"{b}.{a}.{w_}.weight"] = _h(sd[f"{b}.{a}.{w_}.weight"], dev)
                        for k_ in (f"{b}.ff.net.0.proj.weight", f"{b}.ff.net.0.proj.bias", f"{b}.ff.net.2.weight"):
                            self._base_host[k_] = sd[k_].detach().cpu()
                    self.xattn_layers.append(b)
                    # feed forward
                    for k_, v_ in self._ff_weights(b, _f(sd[f"{b}.ff.net.0.proj.weight"], dev),
                                                   _f(sd[f"{b}.ff.net.0.proj.bias"], dev), _f(sd[f"{b}.ff.net.2.weight"], dev)).items():
                        W[k_] = v_
                    W[f"{b}.ff1.b"] = _h(_geglu_interleave(_f(sd[f"{b}.ff.net.0.proj.bias"], dev)), dev)
                    W[f"{b}.ff2.b"] = _h(sd[f"{b}.ff.net.2.bias"], dev)
                if keep_base:
                    for p in ("proj_in", "proj_out"):
                        self._base_host[f"{n}.{p}.weight"] = sd[f"{n}.{p}.weight"].detach().cpu()
                # the last block's ff2 with proj_out as one GEMM (unet._transformer folds where ops.ff2_fold says so)
                W[f"{n}.ffpo.w"], W[f"{n}.ffpo.b"] = fold_ff2_proj_out(W[f"{b}.ff2.w"], W[f"{b}.ff2.b"], W[f"{n}.proj_out.w"],
                                                                       W[f"{n}.proj_out.b"])

    def _ff_weights(self, b: str, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor) -> Dict[str, torch.Tensor]:
        """packed feed-forward weights of transformer block ``b`` from fp32 ``ff.net.0.proj`` (weight, bias) and ``ff.net.2``:
        the GEGLU rows interleaved, norm3 folded into the GEGLU projection (same row interleave for W', s and b')"""
        dev = self.device
        out: Dict[str, torch.Tensor] = {}
        w1i, b1i = _geglu_interleave(w1), _geglu_interleave(b1)
        out[f"{b}.ff1.w"] = _h(w1i, dev)
        out[f"{b}.ff1.wl"], out[f"{b}.ff1.lns"], out[f"{b}.ff1.lnb"] = fold_ln(w1i, self.w[f"{b}.norm3.g"],
                                                                                 self.w[f"{b}.norm3.b"], b1i)
        out[f"{b}.ff2.w"] = _h(w2, dev)
        return out

    def _merged_weight(self, sd, adapter_sd, lora_scale, extra, base: str, idx: int, which: str) -> torch.Tensor:
        """fp32 ``to_q`` / ``to_k`` / ``to_v`` / ``to_out.0`` (``which`` = q, k, v, out) of attention ``base`` as the engine
        merges it: the source weight + lora_scale * the ConsistentID adapter's LoRA of processor ``idx`` + ``extra(path)``"""
        dev = self.device
        path = f"{base}.to_{which}" if which != "out" else f"{base}.to_out.0"
        w = _f(sd[f"{path}.weight"], dev)
        if adapter_sd is not None:
            up = _f(adapter_sd[f"{idx}.to_{which}_lora.up.weight"], dev)
            down = _f(adapter_sd[f"{idx}.to_{which}_lora.down.weight"], dev)
            w = w + lora_scale * (up @ down)
        more = extra(path) if extra is not None else None
        return w if more is None else w + more

    def _attention_weights(self, b: str, d: int, sd, adapter_sd, proc_index, lora_scale, ln2=None, ln1=None,
                           extra=None) -> Dict[str, torch.Tensor]:
        """packed projection weights of transformer block ``b`` (head dim ``d``): LoRA merged in fp32 (attention.py
        :139-162 / :236-282), softmax scale and log2(e) folded into to_q, q/k/v and K/V pairs concatenated.
        ``ln2`` = (gamma, beta) of the block's norm2: where the second-generation fused cross-attention applies
        (cid_id_xattn3_supported), LayerNorm is folded into the query projection (xattn_pack.fold_layernorm); the two
        fp32 fold vectors are stored as raw bits in fp16-typed tensors so that the weight arena stays one dtype.
        ``extra``: module path -> a further fp32 delta or None (``set_lora``), added after the adapter's own LoRA."""
        dev = self.device
        out: Dict[str, torch.Tensor] = {}
        merged = lambda base, idx, which: self._merged_weight(sd, adapter_sd, lora_scale, extra, base, idx, which)

        qscale = (d ** -0.5) * LOG2E
        i1 = proc_index[f"{b}.attn1.processor"]
        qkv = torch.cat([merged(f"{b}.attn1", i1, "q") * qscale, merged(f"{b}.attn1", i1, "k"), merged(f"{b}.attn1", i1, "v")], 0)
        out[f"{b}.attn1.qkv.w"] = _h(qkv, dev)
        if ln1 is not None:     # norm1 folded into the fused q / k / v projection
            out[f"{b}.attn1.qkv.wl"], out[f"{b}.attn1.qkv.lns"], out[f"{b}.attn1.qkv.lnb"] = fold_ln(qkv, ln1[0], ln1[1])
        out[f"{b}.attn1.out.w"] = _h(merged(f"{b}.attn1", i1, "out"), dev)
        i2 = proc_index[f"{b}.attn2.processor"]
        wq2 = merged(f"{b}.attn2", i2, "q") * qscale
        out[f"{b}.attn2.wq"] = _h(wq2, dev)
        if ln2 is not None:     # norm2 folded into the query projection (levels where LN + GEMM + core + GEMM runs)
            out[f"{b}.attn2.wql"], out[f"{b}.attn2.wq_lns"], out[f"{b}.attn2.wq_lnb"] = fold_ln(wq2, ln2[0], ln2[1])
        heads = wq2.shape[0] // d
        if ln2 is not None and ops.id_xattn3_supported(wq2.shape[0], heads, 77, 4):
            from .xattn_pack import fold_layernorm, pack_w3
            wf, qs, qb = fold_layernorm(wq2, ln2[0], ln2[1])
            out[f"{b}.attn2.wq_f"] = wf                                   # (row-major: the comparator build's operand)
            out[f"{b}.attn2.wq_p"] = pack_w3(wf)                          # A-operand streams of the fused kernel
            out[f"{b}.attn2.wo_p"] = pack_w3(_h(merged(f"{b}.attn2", i2, "out"), dev))
            out[f"{b}.attn2.qs"] = qs.view(torch.float16)
            out[f"{b}.attn2.qb"] = qb.view(torch.float16)
        out[f"{b}.attn2.wo"] = _h(merged(f"{b}.attn2", i2, "out"), dev)
        out[f"{b}.attn2.kv_txt.w"] = _h(torch.cat([merged(f"{b}.attn2", i2, "k"), merged(f"{b}.attn2", i2, "v")], 0), dev)
        if adapter_sd is not None:
            kip, vip = adapter_sd[f"{i2}.to_k_ip.weight"], adapter_sd[f"{i2}.to_v_ip.weight"]
        else:  # no adapter: the ID stream is disabled (ip_scale 0); keep shapes valid
            kip, vip = sd[f"{b}.attn2.to_k.weight"], sd[f"{b}.attn2.to_v.weight"]
        out[f"{b}.attn2.kv_ip.w"] = _h(torch.cat([_f(kip, dev), _f(vip, dev)], 0), dev)
        return out

    def load_adapter_modules(self, adapter_sd: Dict[str, torch.Tensor], lora_scale: Optional[float] = None):
        """Merge the ``adapter_modules`` entry of a ConsistentID checkpoint (what the reference does with
        ``ip_layers.load_state_dict(state_dict["adapter_modules"])``, pipline_StableDiffusion_ConsistentID.py:143-144)
        into the packed attention weights IN PLACE: device addresses do not change, so captured step graphs stay
        valid.  Needs ``keep_base=True`` at construction."""
        if not self._base_attn:
            raise RuntimeError("load_adapter_modules needs the base attention weights: construct with keep_base=True")
        from .unet_spec import adapter_param_shapes
        rank = adapter_sd["0.to_q_lora.down.weight"].shape[0] if "0.to_q_lora.down.weight" in adapter_sd else 128
        want = adapter_param_shapes(self.cfg, rank=rank)
        missing = [k for k in want if k not in adapter_sd]
        unexpected = [k for k in adapter_sd if k not in want]
        bad = [k for k in want if k in adapter_sd and tuple(adapter_sd[k].shape) != tuple(want[k])]
        if missing or unexpected or bad:     # the reference loads strict=True
            raise RuntimeError(f"adapter_modules mismatch: missing {missing[:3]} unexpected {unexpected[:3]} shape {bad[:3]}")
        # (kept, so that set_lora can combine both kinds of delta in either load order)
        self._adapter_sd, self._adapter_scale = adapter_sd, self._lora_scale if lora_scale is None else lora_scale
        self._repack_attention(with_ip=True)
        return self

    def _repack_attention(self, with_ip: bool):
        """every packed attention tensor again, in place, from the fp16 base, the kept ConsistentID adapter and the active
        LoRA entries; ``with_ip``: also the ID stream's ``kv_ip`` and ``ip_scale`` (the adapter's part alone)"""
        downs, mid, ups = walk(self.cfg)
        proc_index = {n: i for i, n in enumerate(attn_processor_names(self.cfg))}
        extra = (lambda path: merged_delta(self._lora, path, self.device)) if self._lora else None
        for blk in downs + [mid] + ups:
            for t in blk.attentions:
                for k in range(t.n_layers):
                    b = f"{t.name}.transformer_blocks.{k}"
                    for name, val in self._attention_weights(b, t.channels // t.heads, self._base_attn, self._adapter_sd,
                                                             proc_index, self._adapter_scale,
                                                             ln2=(self.w[f"{b}.norm2.g"], self.w[f"{b}.norm2.b"]),
                                                             ln1=(self.w[f"{b}.norm1.g"], self.w[f"{b}.norm1.b"]),
                                                             extra=extra).items():
                        if with_ip or not name.endswith(".kv_ip.w"):
                            self.w[name].copy_(val)
                    if with_ip:
                        self.ip_scale[b] = 1.0
        self._repack_pag()      # (load_adapter_modules and set_lora both come through here)

    def require_base(self, what: str = "set_lora"):
        """raise the RuntimeError of :meth:`set_lora` now, before a caller changes anything else"""
        if not self._base_attn or not self._base_host:
            raise RuntimeError(f"{what} needs the UNet's base weights: construct with keep_base=True (engines built from the "
                               "broadcast arena do not carry them)")

    def _pag_weights(self, b: str) -> Dict[str, torch.Tensor]:
        """``attn1.vo.*`` of transformer block ``b`` (:func:`fold_vo`) from the fp16 base, the kept ConsistentID adapter and
        the active LoRA entries -- the operands ``_repack_attention`` merges ``attn1.qkv`` / ``attn1.out`` from"""
        proc = {n: i for i, n in enumerate(attn_processor_names(self.cfg))}[f"{b}.attn1.processor"]
        extra = (lambda path: merged_delta(self._lora, path, self.device)) if self._lora else None
        wv, wo = (self._merged_weight(self._base_attn, self._adapter_sd, self._adapter_scale, extra, f"{b}.attn1", proc, which)
                  for which in ("v", "out"))
        wl, s, bias = fold_vo(wv, wo, self.w[f"{b}.norm1.g"], self.w[f"{b}.norm1.b"], self.w[f"{b}.attn1.out.b"])
        return dict(zip((f"{b}.attn1.vo.{x}" for x in PAG_SUFFIXES), (_h(wo @ wv, self.device), wl, s, bias)))

    def _repack_pag(self):
        for b in self._pag_blocks:
            for name, val in self._pag_weights(b).items():
                self.pag[name].copy_(val)

    def set_pag(self, blocks):
        """The transformer blocks whose ``attn1`` perturbed-attention guidance replaces by identity attention -> ``self.pag``
        holds their ``attn1.vo.{w,wl,lns,lnb}`` and nothing else.  A block that stays selected keeps its tensors (and their
        addresses); they follow every later ``load_adapter_modules`` / ``set_lora`` in place.  Built from the un-merged base:
        needs ``keep_base=True`` at construction, like ``set_lora``."""
        blocks = tuple(dict.fromkeys(blocks))
        if blocks:
            self.require_base("enable_pag")
        for b in self._pag_blocks:
            if b not in blocks:
                for x in PAG_SUFFIXES:
                    del self.pag[f"{b}.attn1.vo.{x}"]
        for b in blocks:
            if b not in self._pag_blocks:
                self.pag.update(self._pag_weights(b))
        self._pag_blocks = blocks
        return self

    def set_lora(self, entries):
        """Merge community LoRA deltas IN PLACE (lora.py): ``entries`` is the list of active ``(modules, weight)`` with
        ``modules`` = {module path: (down, up, alpha)}.  Every LoRA-able weight is recomputed in fp32 as
        base + lora_scale * up_cid @ down_cid + sum_a weight_a * delta_a (entries summed in their order), pushed through the
        packing of the constructor and copied into the existing tensors: ``attn1.qkv.{w,wl,lns,lnb}``, ``attn1.out.w``,
        ``attn2.{wq,wql,wq_lns,wq_lnb,wq_f,wq_p,qs,qb,wo,wo_p,kv_txt.w}``, ``ff1.{w,wl,lns,lnb}``, ``ff2.w``, ``proj_in.w``,
        ``proj_out.w`` and ``ffpo.{w,b}``.  Biases and ``kv_ip`` do not change, and no address does.  ``set_lora([])``
        restores the base (with the ConsistentID adapter, if one is loaded) bit for bit; an entry of weight 0 counts as
        absent, so that -0.0 + 0.0 cannot flip a sign bit.  Needs ``keep_base=True`` at construction."""
        self.require_base()
        self._lora = [(modules, float(weight)) for modules, weight in entries if float(weight) != 0.0]
        dev, W = self.device, self.w

        def more(path: str, w: torch.Tensor) -> torch.Tensor:
            d = merged_delta(self._lora, path, dev)
            return w if d is None else w + d

        self._repack_attention(with_ip=False)
        downs, mid, ups = walk(self.cfg)
        for blk in downs + [mid] + ups:
            for t in blk.attentions:
                n, c = t.name, t.channels
                for p in ("proj_in", "proj_out"):
                    W[f"{n}.{p}.w"].copy_(_h(more(f"{n}.{p}", _f(self._base_host[f"{n}.{p}.weight"], dev).reshape(c, c)), dev))
                for k in range(t.n_layers):
                    b = f"{n}.transformer_blocks.{k}"
                    ff = self._ff_weights(b, more(f"{b}.ff.net.0.proj", _f(self._base_host[f"{b}.ff.net.0.proj.weight"], dev)),
                                          _f(self._base_host[f"{b}.ff.net.0.proj.bias"], dev),
                                          more(f"{b}.ff.net.2", _f(self._base_host[f"{b}.ff.net.2.weight"], dev)))
                    for name, val in ff.items():
                        W[name].copy_(val)
                w, bias = fold_ff2_proj_out(W[f"{b}.ff2.w"], W[f"{b}.ff2.b"], W[f"{n}.proj_out.w"], W[f"{n}.proj_out.b"])
                W[f"{n}.ffpo.w"].copy_(w)
                W[f"{n}.ffpo.b"].copy_(bias)
        return self

    def retained_device_bytes(self) -> int:
        """device bytes kept beside the packed tensors for later merges (the fp16 attention base of ``keep_base``)"""
        kept = list(self._base_attn.values()) + list(self._base_host.values()) + list((self._adapter_sd or {}).values())
        return sum(t.numel() * t.element_size() for t in kept if t.is_cuda)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.w.values())

    # ---- export / import for the one-off RCCL weight broadcast (distributed.broadcast_weights)
    def meta(self) -> dict:
        m = dict(temb_offsets=self.temb_offsets, temb_total=self.temb_total, ip_scale=self.ip_scale,
                 xattn_layers=self.xattn_layers, encoder_only=self.encoder_only, lora_scale=self._lora_scale)
        if self.encoder_only:
            m.update(cond_convs=self.cond_convs, n_zero=self.n_zero)
        return m

    @classmethod
    def from_tensors(cls, cfg: UNetConfig, w: Dict[str, torch.Tensor], meta: dict, device) -> "PackedUNet":
        self = cls.__new__(cls)
        self.cfg, self.device, self.w = cfg, device, w
        self._base_attn, self._lora_scale = {}, meta.get("lora_scale", 1.0)   # (un-merged weights are not broadcast)
        self._base_host, self._lora, self._adapter_sd, self._adapter_scale = {}, [], None, self._lora_scale
        self.pag, self._pag_blocks = {}, ()
        self.temb_offsets, self.temb_total = meta["temb_offsets"], meta["temb_total"]
        self.ip_scale, self.xattn_layers = meta["ip_scale"], meta["xattn_layers"]
        self.encoder_only = meta.get("encoder_only", False)
        if self.encoder_only:
            self.cond_convs, self.n_zero = meta["cond_convs"], meta["n_zero"]
        return self
