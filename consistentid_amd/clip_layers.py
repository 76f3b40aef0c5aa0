"""The CLIP encoder layer both towers run (clip_text.py, clip_vision.py): its weight packing and its launch sequence.

A layer is LayerNorm -> fused QKV GEMM (V written transposed, softmax scale x log2 e folded into the Q rows) -> attention
-> out-proj GEMM (+residual) -> LayerNorm -> fc1 GEMM -> activation in place -> fc2 GEMM (+residual), on a token axis
padded to a multiple of 64.  The towers differ in the attention kernel only (``ops.self_attn_causal`` over T real tokens
for text, ``ops.self_attn`` over the real keys for vision) and pass it in; embeddings, the norms around the stack,
projections and pooling stay with the towers.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .weights import LOG2E, _h

# ``hidden_act`` -> the in-place kernel (exact GELU: ViT-H, OpenCLIP bigG; quick GELU: CLIP-L, the safety checker's ViT-L)
ACTIVATIONS = {"quick_gelu": ops.quick_gelu_, "gelu": ops.gelu_}


def pack_layers(W: Dict[str, torch.Tensor], sd: Dict[str, torch.Tensor], n_layers: int, d: int, dev) -> None:
    """``encoder.layers.{i}.*`` of a transformers state dict -> fp16 ``W["{i}.qkv.w"]``, ``{i}.o.w``, ``{i}.layer_norm1.g``,
    ``{i}.fc1.w`` ... (and the biases) for heads of width ``d``"""
    qs = (d ** -0.5) * LOG2E                                             # CLIPAttention.scale and log2 e
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        a = p + "self_attn."
        W.update(pack_layer_weights(lambda k: sd[k].float(), i, d, dev))
        W[f"{i}.qkv.b"] = _h(torch.cat([sd[a + "q_proj.bias"].float() * qs, sd[a + "k_proj.bias"].float(),
                                        sd[a + "v_proj.bias"].float()], 0), dev)
        W[f"{i}.o.b"] = _h(sd[a + "out_proj.bias"], dev)
        for ln in ("layer_norm1", "layer_norm2"):
            W[f"{i}.{ln}.g"], W[f"{i}.{ln}.b"] = _h(sd[p + ln + ".weight"], dev), _h(sd[p + ln + ".bias"], dev)
        for fc in ("fc1", "fc2"):
            W[f"{i}.{fc}.b"] = _h(sd[p + f"mlp.{fc}.bias"], dev)


def pack_layer_weights(get, i: int, d: int, dev) -> Dict[str, torch.Tensor]:
    """the four weight matrices of layer ``i`` -- ``{i}.qkv.w`` (scale folded into the Q rows), ``{i}.o.w``, ``{i}.fc1.w``,
    ``{i}.fc2.w`` -- from ``get(key)``, which returns the fp32 weight of ``encoder.layers.{i}.<linear>.weight`` on the host
    (the state dict's own, or with LoRA deltas merged: ``HipCLIPTextModel.set_lora``)"""
    qs = (d ** -0.5) * LOG2E
    p = f"encoder.layers.{i}."
    a = p + "self_attn."
    return {f"{i}.qkv.w": _h(torch.cat([get(a + "q_proj.weight") * qs, get(a + "k_proj.weight"), get(a + "v_proj.weight")], 0),
                             dev),
            f"{i}.o.w": _h(get(a + "out_proj.weight"), dev), f"{i}.fc1.w": _h(get(p + "mlp.fc1.weight"), dev),
            f"{i}.fc2.w": _h(get(p + "mlp.fc2.weight"), dev)}


def run_layer(W: Dict[str, torch.Tensor], i: int, x: torch.Tensor, *, B: int, Np: int, heads: int, d: int, eps: float,
              attn, n_keys: int, act) -> torch.Tensor:
    """layer ``i`` on ``x`` [B * Np, C] (Np: the padded token axis) -> a new [B * Np, C]; ``attn``: the attention function,
    which sees ``n_keys`` real keys; ``act``: the tower's entry of ``ACTIVATIONS``"""
    M, C = x.shape
    empty = lambda *shape: torch.empty(*shape, dtype=torch.float16, device=x.device)
    ln = empty(M, C)
    ops.layernorm(x, ln, W[f"{i}.layer_norm1.g"], W[f"{i}.layer_norm1.b"], M=M, C_=C, eps=eps)
    qk = empty(M, 2 * C)
    vt = empty(B * heads * ops.dvp_of(d) * Np)
    ops.gemm(ln, W[f"{i}.qkv.w"], qk, M=M, N=3 * C, c1=C, bias=W[f"{i}.qkv.b"], mode=2, vt=vt, n_vt0=2 * C,
             heads=heads, dhead=d, ntok=Np)
    ao = empty(M, C)
    attn(qk, qk[:, C:], vt, ao, B=B, N=Np, heads=heads, d=d, ldq=2 * C, ldk=2 * C, ldo=C, n_keys=n_keys)
    x2 = empty(M, C)
    ops.gemm(ao, W[f"{i}.o.w"], x2, M=M, N=C, c1=C, bias=W[f"{i}.o.b"], res=x, ldr=C)
    ln2 = empty(M, C)
    ops.layernorm(x2, ln2, W[f"{i}.layer_norm2.g"], W[f"{i}.layer_norm2.b"], M=M, C_=C, eps=eps)
    f = empty(M, W[f"{i}.fc1.w"].shape[0])
    ops.gemm(ln2, W[f"{i}.fc1.w"], f, M=M, N=f.shape[1], c1=C, bias=W[f"{i}.fc1.b"])
    act(f)
    out = empty(M, C)
    ops.gemm(f, W[f"{i}.fc2.w"], out, M=M, N=C, c1=f.shape[1], bias=W[f"{i}.fc2.b"], res=x2, ldr=C)
    return out
