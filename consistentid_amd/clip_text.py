"""HIP execution engine for the CLIP text towers as the reference uses them (once per prompt):

    self.text_encoder(clean_input_id)[0]                                   SD1.5 pipline_StableDiffusion_ConsistentID.py:467
    self._encode_prompt(...)  -> text_encoder(ids)[0]                      SD1.5 :469-475 (D: encode_prompt), inpaint, CN
    self.text_encoder(ids, output_hidden_states=True).hidden_states[-2]    SDXL pipline_StableDiffusionXL_ConsistentID.py:514
    self.text_encoder_2(ids2, output_hidden_states=True) -> [0], .hidden_states[-2]                               SDXL :519-521

``HipCLIPTextModel`` stands in for transformers' ``CLIPTextModel`` (SD1.5's CLIP-L, SDXL's first tower) and
``CLIPTextModelWithProjection`` (SDXL's OpenCLIP bigG, ``text_projection.weight`` present).  Weights: the transformers
state_dict (``text_model.*`` + ``text_projection.weight``; keys without the ``text_model.`` prefix are read as well).
Every layer is the encoder layer of clip_layers.py (weights packed and launched there) around
``cid_self_attn_causal_f16`` (T real tokens on a token axis padded to a multiple of 64); the embedding is
``cid_text_embed_f16``, the projection ``cid_linear_small_f16``.  Pad rows of the token axis start at zero and stay
row-local.  The host-side rules (config mapping, the id check, the EOS pooling index) are plain functions below, so that
they can be tested without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .clip_layers import ACTIVATIONS, pack_layer_weights, pack_layers, run_layer
from .lora import TOWER_MODULES, merged_delta
from .weights import _h


@dataclass(frozen=True)
class TextTowerConfig:
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    max_position_embeddings: int
    vocab_size: int
    hidden_act: str
    layer_norm_eps: float
    eos_token_id: int
    projection_dim: Optional[int]

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


def text_config(config) -> TextTowerConfig:
    """transformers ``CLIPTextConfig`` (or its ``config.json`` as a dict) -> TextTowerConfig; refuses what the engine does
    not build.  Defaults are CLIPTextConfig's."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    act = get("hidden_act", "quick_gelu")
    if act not in ACTIVATIONS:
        raise NotImplementedError(f"hidden_act {act!r}: the text towers are built with {tuple(ACTIVATIONS)}")
    cfg = TextTowerConfig(
        hidden_size=int(get("hidden_size", 512)), intermediate_size=int(get("intermediate_size", 2048)),
        num_hidden_layers=int(get("num_hidden_layers", 12)), num_attention_heads=int(get("num_attention_heads", 8)),
        max_position_embeddings=int(get("max_position_embeddings", 77)), vocab_size=int(get("vocab_size", 49408)),
        hidden_act=act, layer_norm_eps=float(get("layer_norm_eps", 1e-5)), eos_token_id=int(get("eos_token_id", 49407)),
        projection_dim=get("projection_dim"))
    if cfg.hidden_size % cfg.num_attention_heads or cfg.head_dim != 64:
        raise NotImplementedError(f"hidden_size {cfg.hidden_size} / {cfg.num_attention_heads} heads: the causal attention "
                                  "kernel is built for 64-wide heads (CLIP-L, OpenCLIP bigG)")
    return cfg


def check_ids(input_ids: torch.Tensor, vocab_size: int) -> None:
    """Every id must index the token table.  The trigger tokens that load_ConsistentID_model adds to the tokenizer
    (<|image|> 49408, <|facial|> 49409) lie outside it: the reference never resizes the table, so a prompt that still holds
    one cannot be embedded -- this raises instead of reading past the table."""
    ids = input_ids.detach().to("cpu", torch.long)
    bad = (ids < 0) | (ids >= vocab_size)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise ValueError(f"token id {int(ids.flatten()[i])} is outside the text encoder's embedding table (vocab size "
                         f"{vocab_size}); trigger tokens such as <|image|> / <|facial|> must be removed from the ids first "
                         "(encode_prompt_with_trigger_word does)")


def pool_index(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """The row of each sequence that ``pooler_output`` takes, transformers' rule exactly: with the legacy
    ``eos_token_id == 2`` of the SD1.5 / SDXL configs the largest id (argmax, first on ties), else the first position of
    ``eos_token_id``.  Host tensor [B] (long)."""
    ids = input_ids.detach().to("cpu", torch.long)
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1).long()
    return (ids.to(torch.int) == eos_token_id).int().argmax(dim=-1).long()


class TextEncoderOutput:
    """transformers-style output: attribute access and ``[i]`` over the fields that are set, in the model's order
    (``CLIPTextModel``: last_hidden_state, pooler_output, hidden_states; ``CLIPTextModelWithProjection``: text_embeds,
    last_hidden_state, hidden_states -- its ``pooler_output`` is kept as an attribute only)."""

    def __init__(self, order, **fields):
        self.__dict__.update(fields)
        self._tuple = tuple(fields[k] for k in order if fields.get(k) is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self._tuple[i]

    def __len__(self):
        return len(self._tuple)

    def to_tuple(self):
        return self._tuple


class HipCLIPTextModel:
    def __init__(self, state_dict: Dict[str, torch.Tensor], config, device="cuda:0", keep_base: bool = False):
        """``keep_base``: keep references to the state dict's six LoRA-able weights per layer on the HOST (no device
        memory), so that ``set_lora`` can merge community LoRA files later, in place"""
        self.config = config
        self.spec = cfg = text_config(config)
        self.device = dev = torch.device(device)
        self.dtype = torch.float16
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()
              if not k.endswith("position_ids")}
        self.with_projection = "text_projection.weight" in sd
        C = cfg.hidden_size
        self.C, self.heads, self.d, self.eps = C, cfg.num_attention_heads, cfg.head_dim, cfg.layer_norm_eps
        self.tok = _h(sd["embeddings.token_embedding.weight"], dev)           # [V, C]
        self.pos = _h(sd["embeddings.position_embedding.weight"], dev)        # [P, C]
        if tuple(self.tok.shape) != (cfg.vocab_size, C) or tuple(self.pos.shape) != (cfg.max_position_embeddings, C):
            raise ValueError(f"embedding tables {tuple(self.tok.shape)} / {tuple(self.pos.shape)} do not match the config "
                             f"(vocab {cfg.vocab_size}, {cfg.max_position_embeddings} positions, width {C})")
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
        if n_layers != cfg.num_hidden_layers:
            raise ValueError(f"{n_layers} encoder layers in the weights, {cfg.num_hidden_layers} in the config")
        self.n_layers = n_layers
        self._act = ACTIVATIONS[cfg.hidden_act]
        W: Dict[str, torch.Tensor] = {"final.g": _h(sd["final_layer_norm.weight"], dev),
                                      "final.b": _h(sd["final_layer_norm.bias"], dev)}
        pack_layers(W, sd, n_layers, self.d, dev)
        if self.with_projection:
            W["proj.w"] = _h(sd["text_projection.weight"], dev)                # [projection_dim, C], no bias
        self.W = W
        self._base: Dict[str, torch.Tensor] = {}
        if keep_base:
            for i in range(n_layers):
                for m in TOWER_MODULES:
                    self._base[f"encoder.layers.{i}.{m}.weight"] = sd[f"encoder.layers.{i}.{m}.weight"].detach().cpu()

    def require_base(self):
        """raise the RuntimeError of :meth:`set_lora` now, before a caller changes anything else"""
        if not self._base:
            raise RuntimeError("LoRA weights need the text tower's base weights: construct HipCLIPTextModel with keep_base=True")

    def set_lora(self, entries):
        """the active community LoRA entries ``[(modules, weight), ...]`` (lora.parse_lora's part for this tower; module
        paths ``text_model.encoder.layers.{i}.<linear>``) -> ``{i}.qkv.w`` (scale folded into the Q rows), ``{i}.o.w``,
        ``{i}.fc1.w`` and ``{i}.fc2.w``, recomputed in fp32 on the host as base + sum_a weight_a * delta_a and copied into the
        existing device tensors.  ``[]`` restores the base bit for bit; an entry of weight 0 counts as absent."""
        self.require_base()
        entries = [(modules, float(weight)) for modules, weight in entries if float(weight) != 0.0]

        def get(key: str) -> torch.Tensor:
            w = self._base[key].float()
            d = merged_delta(entries, "text_model." + key[:-len(".weight")])
            return w if d is None else w + d

        for i in range(self.n_layers):
            for name, val in pack_layer_weights(get, i, self.d, self.device).items():
                self.W[name].copy_(val)
        return self

    def _empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float16, device=self.device)

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, output_hidden_states: bool = False, **kwargs):
        from . import ops
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: the reference's text encoder calls pass none (CLIP towers attend "
                                      "causally over the padded 77 tokens)")
        if kwargs.get("position_ids") is not None:
            raise NotImplementedError("position_ids: positions are 0 .. T-1")
        ids = torch.as_tensor(input_ids)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        B, T = ids.shape
        cfg, W, C, dev = self.spec, self.W, self.C, self.device
        if not 0 < T <= cfg.max_position_embeddings:
            raise ValueError(f"sequence length {T}: the position table holds {cfg.max_position_embeddings}")
        check_ids(ids, cfg.vocab_size)
        pidx = pool_index(ids, cfg.eos_token_id)
        Tp = (T + 63) // 64 * 64                                         # padded token axis
        M = B * Tp
        x = self._empty(M, C)
        ops.text_embed(ids.to(device=dev, dtype=torch.int32).contiguous(), self.tok, self.pos, x, B=B, T=T, Tp=Tp)
        states = [x]
        for i in range(self.n_layers):
            x = run_layer(W, i, x, B=B, Np=Tp, heads=self.heads, d=self.d, eps=self.eps, attn=ops.self_attn_causal,
                          n_keys=T, act=self._act)
            states.append(x)
        last = self._empty(M, C)
        ops.layernorm(x, last, W["final.g"], W["final.b"], M=M, C_=C, eps=self.eps)
        unpad = lambda t: t.view(B, Tp, C)[:, :T].contiguous()
        last_hidden_state = unpad(last)
        pooled = last_hidden_state[torch.arange(B, device=dev), pidx.to(dev)].contiguous()      # row gather (plumbing)
        hidden_states = tuple(unpad(s) for s in states) if output_hidden_states else None
        if not self.with_projection:
            return TextEncoderOutput(("last_hidden_state", "pooler_output", "hidden_states"),
                                     last_hidden_state=last_hidden_state, pooler_output=pooled, hidden_states=hidden_states)
        P = W["proj.w"].shape[0]
        text_embeds = self._empty(B, P)
        for m0 in range(0, B, 64):                                       # cid_linear_small_f16 takes up to 64 rows
            mb = min(64, B - m0)
            ops.linear_small(pooled[m0:m0 + mb], W["proj.w"], None, text_embeds[m0:m0 + mb], M=mb, N=P, K=C)
        return TextEncoderOutput(("text_embeds", "last_hidden_state", "hidden_states"), text_embeds=text_embeds,
                                 last_hidden_state=last_hidden_state, hidden_states=hidden_states, pooler_output=pooled)
