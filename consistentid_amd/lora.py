"""Community LoRA files for the UNet and the text towers: reading, key spellings, validation and the weight deltas.

The reference scripts' block "using LoRA modules in community" (infer.py, infer_SDXL.py):

    pipe.load_lora_weights(os.path.dirname(lora_path), weight_name=lora_model_name)
    pipe.set_adapters([...], adapter_weights=[...])
    pipe.fuse_lora()

The engine has no ``nn.Linear`` to wrap: its weights exist only packed (weights.py, clip_layers.py).  A LoRA is therefore
parsed here into ``{module path: (down, up, alpha)}`` per target (``unet``, ``text_encoder``, ``text_encoder_2``) and merged
into the un-packed base weights by ``PackedUNet.set_lora`` / ``HipCLIPTextModel.set_lora``, which repack in place.

Two families of key spellings are read, per key:
  kohya      ``lora_unet_<name>`` / ``lora_te_<name>`` / ``lora_te1_<name>`` / ``lora_te2_<name>`` with the suffixes
             ``.lora_down.weight``, ``.lora_up.weight`` and an optional scalar ``.alpha``; ``<name>`` is the module path with
             every ``.`` written as ``_``.  It is looked up in a table built from the model's configuration (module paths
             hold underscores of their own, so the name is never split).  SDXL files name UNet blocks in the original
             numbering (``input_blocks_N_M``, ``middle_block_M``, ``output_blocks_N_M``): ``sgm_block_names`` derives it.
  diffusers  ``unet.<path>`` / ``text_encoder.<path>`` / ``text_encoder_2.<path>`` with ``.lora_A.weight`` / ``.lora_B.weight``
             (peft), ``.lora.down.weight`` / ``.lora.up.weight`` or ``.lora_linear_layer.down.weight`` / ``.up.weight``; no
             alpha, so the scale is 1.

Everything is validated on the whole file before a weight is touched (``parse_lora``).  Pure host code.
"""
from __future__ import annotations

import os
import warnings
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple, Union

import torch

from .unet_spec import UNetConfig, unet_param_shapes, walk

TARGETS = ("unet", "text_encoder", "text_encoder_2")

# LoRA-able linears of a BasicTransformerBlock (a Transformer2DModel adds its proj_in / proj_out) and of a CLIP encoder layer
BLOCK_MODULES = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
                 "attn2.to_out.0", "ff.net.0.proj", "ff.net.2")
TOWER_MODULES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")

KOHYA_PREFIXES = (("lora_unet_", "unet"), ("lora_te1_", "text_encoder"), ("lora_te2_", "text_encoder_2"),
                  ("lora_te_", "text_encoder"))
KOHYA_SUFFIXES = ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha"))
DIFFUSERS_PREFIXES = (("unet.", "unet"), ("text_encoder_2.", "text_encoder_2"), ("text_encoder.", "text_encoder"))
DIFFUSERS_SUFFIXES = ((".lora_A.weight", "down"), (".lora_B.weight", "up"),
                      (".lora_linear_layer.down.weight", "down"), (".lora_linear_layer.up.weight", "up"),
                      (".lora.down.weight", "down"), (".lora.up.weight", "up"))
# other parametrisations (LoHa, LoKr, LoCon's mid tensor, DoRA, full differences, trained biases): not built
FOREIGN_MARKS = ("hada_", "lokr_", "lora_mid", "dora_scale", "lora_magnitude_vector")
FOREIGN_SUFFIXES = (".diff", ".diff_b", ".bias")
# what the original (SGM) numbering calls the parts of the UNet that take no LoRA here: the time / label embeddings and the
# output convolution, and inside its numbered blocks the resnets' convolutions and time projections and the samplers
SGM_BLOCKS = ("input_blocks_", "middle_block_", "output_blocks_")
SGM_ENDS = ("time_embed_", "label_emb_", "out_")
SGM_OTHER_PARTS = ("_in_layers_", "_out_layers_", "_emb_layers_")
SGM_OTHER_TAILS = ("_skip_connection", "_op", "_conv")


def _sgm_other(name: str) -> bool:
    return name.startswith(SGM_ENDS) or (name.startswith(SGM_BLOCKS) and (name.endswith(SGM_OTHER_TAILS)
                                                                         or any(p in name for p in SGM_OTHER_PARTS)))


Modules = Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[float]]]


# ------------------------------------------------------------------------------------------------ module tables
def unet_modules(cfg: UNetConfig) -> "OrderedDict[str, Tuple[int, int]]":
    """every LoRA-able module path of the UNet -> (out features, in features)"""
    shapes = unet_param_shapes(cfg)
    out: "OrderedDict[str, Tuple[int, int]]" = OrderedDict()
    downs, mid, ups = walk(cfg)
    for blk in downs + [mid] + ups:
        for t in blk.attentions:
            paths = [f"{t.name}.proj_in"]
            for k in range(t.n_layers):
                paths += [f"{t.name}.transformer_blocks.{k}.{m}" for m in BLOCK_MODULES]
            paths.append(f"{t.name}.proj_out")
            for p in paths:
                out[p] = tuple(shapes[f"{p}.weight"][:2])
    return out


def unet_other_modules(cfg: UNetConfig) -> List[str]:
    """the weight-bearing module paths of the UNet that take NO LoRA here (3x3 convolutions, conv_in / conv_out /
    conv_shortcut, time_emb_proj, time_embedding, add_embedding): a key that addresses one is refused by name"""
    lorable = unet_modules(cfg)
    return [k[:-len(".weight")] for k, s in unet_param_shapes(cfg).items()
            if k.endswith(".weight") and len(s) >= 2 and k[:-len(".weight")] not in lorable]


def tower_modules(n_layers: int, hidden: Optional[int] = None, intermediate: Optional[int] = None
                  ) -> "OrderedDict[str, Optional[Tuple[int, int]]]":
    """every LoRA-able module path of a CLIP text tower (transformers names, ``text_model.encoder.layers.{i}...``) ->
    (out features, in features), or None where the widths are not given"""
    out: "OrderedDict[str, Optional[Tuple[int, int]]]" = OrderedDict()
    for i in range(n_layers):
        for m in TOWER_MODULES:
            shape = None
            if hidden is not None and intermediate is not None:
                shape = {"mlp.fc1": (intermediate, hidden), "mlp.fc2": (hidden, intermediate)}.get(m, (hidden, hidden))
            out[f"text_model.encoder.layers.{i}.{m}"] = shape
    return out


def kohya_name(path: str) -> str:
    """module path -> the name kohya's scripts write: every ``.`` becomes ``_``"""
    return path.replace(".", "_")


def sgm_block_names(cfg: UNetConfig) -> Dict[str, str]:
    """diffusers block part -> its name in the original numbering, derived from the configuration:
    ``input_blocks.0`` is conv_in; every down block then contributes one entry per layer, [resnet, attention?], and one for
    its downsampler; ``middle_block`` is [resnet 0, attention 0, resnet 1]; every up block contributes
    ``layers_per_block + 1`` entries [resnet, attention?, upsampler?]."""
    downs, mid, ups = walk(cfg)
    names: Dict[str, str] = {}
    n = 0
    for blk in downs:
        for j, r in enumerate(blk.resnets):
            n += 1
            names[r.name] = f"input_blocks.{n}.0"
            if blk.attentions:
                names[blk.attentions[j].name] = f"input_blocks.{n}.1"
        if blk.sampler:
            n += 1
            names[f"{blk.name}.{blk.sampler}"] = f"input_blocks.{n}.0"
    names[mid.resnets[0].name], names[mid.attentions[0].name] = "middle_block.0", "middle_block.1"
    names[mid.resnets[1].name] = "middle_block.2"
    n = 0
    for blk in ups:
        for j, r in enumerate(blk.resnets):
            names[r.name] = f"output_blocks.{n}.0"
            if blk.attentions:
                names[blk.attentions[j].name] = f"output_blocks.{n}.1"
            if blk.sampler and j == len(blk.resnets) - 1:
                names[f"{blk.name}.{blk.sampler}"] = f"output_blocks.{n}.{2 if blk.attentions else 1}"
            n += 1
    return names


def sgm_path(cfg: UNetConfig, path: str) -> str:
    """LoRA-able module path (diffusers) -> the same module in the original numbering"""
    for part, name in sgm_block_names(cfg).items():
        if path.startswith(part + "."):
            return name + path[len(part):]
    raise KeyError(path)


def unet_name_table(cfg: UNetConfig, sgm: bool = False) -> Dict[str, str]:
    """kohya name (without ``lora_unet_``) -> module path, over all LoRA-able modules; ``sgm``: the original numbering"""
    return {kohya_name(sgm_path(cfg, p) if sgm else p): p for p in unet_modules(cfg)}


def tower_name_table(n_layers: int) -> Dict[str, str]:
    """kohya name (without ``lora_te_`` / ``lora_te1_`` / ``lora_te2_``) -> module path of a text tower"""
    return {kohya_name(p): p for p in tower_modules(n_layers)}


# ------------------------------------------------------------------------------------------------ the file
def read_lora(path_or_dict: Union[str, os.PathLike, Dict[str, torch.Tensor]], weight_name: Optional[str] = None
              ) -> Dict[str, torch.Tensor]:
    """A LoRA as a flat ``{key: tensor}``: a dict, a ``.safetensors`` file, a ``.bin`` / ``.pt`` file (``weights_only``), or
    a folder plus ``weight_name``.  Local files only; a path that does not exist raises FileNotFoundError."""
    if isinstance(path_or_dict, dict):
        return dict(path_or_dict)
    path = os.fspath(path_or_dict)
    if os.path.isdir(path):
        if not weight_name:
            raise ValueError(f"{path} is a folder: name the file with weight_name=")
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: LoRA files are read from the local file system (hub ids are not resolved)")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a flat dict of tensors, found {type(sd).__name__}")
    return sd


def _split_key(key: str):
    """-> (spelling, target, name, role, prefix) of a key in one of the known spellings, else None"""
    for prefixes, suffixes, spelling in ((KOHYA_PREFIXES, KOHYA_SUFFIXES, "kohya"),
                                         (DIFFUSERS_PREFIXES, DIFFUSERS_SUFFIXES, "diffusers")):
        for prefix, target in prefixes:
            if key.startswith(prefix):
                for suffix, role in suffixes:
                    if key.endswith(suffix):
                        return spelling, target, key[len(prefix):len(key) - len(suffix)], role, prefix
                break
    return None


def _is_foreign(key: str) -> bool:
    return any(m in key for m in FOREIGN_MARKS) or key.endswith(FOREIGN_SUFFIXES)


def _name3(keys: List[str]) -> str:
    return ", ".join(repr(k) for k in keys[:3]) + (f" (and {len(keys) - 3} more)" if len(keys) > 3 else "")


def parse_lora(flat: Dict[str, torch.Tensor], cfg: UNetConfig, towers: Optional[Dict[str, object]] = None
               ) -> Dict[str, Modules]:
    """Normalise and validate a whole LoRA: ``{target: {module path: (down [r, in], up [out, r], alpha or None)}}``.

    ``towers``: ``{"text_encoder": spec, "text_encoder_2": spec}`` of the towers the pipeline holds (anything with
    ``num_hidden_layers``, ``hidden_size`` and ``intermediate_size``; None or absent: no such tower).  Keys of a tower
    that is not there are skipped with one UserWarning per prefix.  Raises NotImplementedError for keys of another
    parametrisation and for keys that address a module without LoRA support, ValueError for keys in no known spelling,
    a ``down`` without its ``up`` (or the reverse) and shapes that do not fit -- all before anything is returned."""
    towers = towers or {}
    foreign = [k for k in flat if _is_foreign(k)]
    if foreign:
        raise NotImplementedError(f"LoRA keys of another parametrisation (LoHa / LoKr / DoRA / full differences / biases are "
                                  f"not built): {_name3(foreign)}")
    shapes = {"unet": unet_modules(cfg)}
    names = {"unet": {**unet_name_table(cfg), **unet_name_table(cfg, sgm=True)}}
    other = {kohya_name(p): p for p in unet_other_modules(cfg)}
    for target in TARGETS[1:]:
        spec = towers.get(target)
        if spec is not None:
            shapes[target] = tower_modules(spec.num_hidden_layers, spec.hidden_size, spec.intermediate_size)
            names[target] = tower_name_table(spec.num_hidden_layers)
    unknown, unsupported, skipped = [], [], OrderedDict()
    parts: Dict[Tuple[str, str], Dict[str, torch.Tensor]] = OrderedDict()
    for key, tensor in flat.items():
        split = _split_key(key)
        if split is None:
            unknown.append(key)
            continue
        spelling, target, name, role, prefix = split
        if target not in shapes:                    # a tower the pipeline does not hold
            skipped.setdefault(prefix, target)
            continue
        if spelling == "kohya":
            path = names[target].get(name)
            if path is None:
                if target == "unet" and (name in other or _sgm_other(name)):
                    unsupported.append(key)
                else:
                    unknown.append(key)
                continue
        else:
            path = name
            if target != "unet" and not path.startswith("text_model."):
                path = "text_model." + path
            if path not in shapes[target]:
                (unsupported if target == "unet" and path in other.values() else unknown).append(key)
                continue
        parts.setdefault((target, path), {})[role] = tensor
    if unsupported:
        raise NotImplementedError(f"LoRA on modules that take none here (3x3 convolutions, conv_in / conv_out / conv_shortcut, "
                                  f"time_emb_proj, time_embedding, add_embedding): {_name3(unsupported)}")
    if unknown:
        raise ValueError(f"LoRA keys in no known spelling (kohya lora_unet_ / lora_te_ / lora_te1_ / lora_te2_, diffusers "
                         f"unet. / text_encoder. / text_encoder_2.) or of no module of this model: {_name3(unknown)}")
    out: Dict[str, Modules] = {t: OrderedDict() for t in TARGETS}
    for (target, path), p in parts.items():
        lack = [r for r in ("down", "up") if r not in p]
        if lack:
            raise ValueError(f"LoRA module {target}.{path}: {' / '.join(sorted(p))} without its {' / '.join(lack)}")
        down, up = p["down"], p["up"]
        if down.dim() == 4 and tuple(down.shape[2:]) == (1, 1) and up.dim() == 4 and tuple(up.shape[2:]) == (1, 1):
            down, up = down.flatten(1), up.flatten(1)       # 1x1 convolutions (SD1.5 proj_in / proj_out)
        want = shapes[target][path]
        if (down.dim() != 2 or up.dim() != 2 or down.shape[0] != up.shape[1]
                or (want is not None and (up.shape[0], down.shape[1]) != tuple(want))):
            raise ValueError(f"LoRA module {target}.{path}: down {tuple(p['down'].shape)} / up {tuple(p['up'].shape)} do not "
                             f"fit the module's weight {want} or each other")
        alpha = p.get("alpha")
        out[target][path] = (down, up, None if alpha is None else float(alpha))
    for prefix, target in skipped.items():
        warnings.warn(f"LoRA keys {prefix}* skipped: the pipeline has no {target}", UserWarning, stacklevel=2)
    return out


def delta(down: torch.Tensor, up: torch.Tensor, alpha: Optional[float], device=None) -> torch.Tensor:
    """``(alpha / r if alpha is given else 1) * up @ down`` in fp32 (r = ``down.shape[0]``), on ``device`` (default: where
    ``down`` lives)"""
    device = down.device if device is None else device
    d = up.to(device=device, dtype=torch.float32) @ down.to(device=device, dtype=torch.float32)
    return d if alpha is None else d * (alpha / down.shape[0])


def merged_delta(entries, path: str, device=None) -> Optional[torch.Tensor]:
    """sum over the active ``(modules, weight)`` entries, in their order, of ``weight * delta`` for module ``path``; None
    where no entry touches it"""
    total = None
    for modules, weight in entries:
        if path in modules:
            d = delta(*modules[path], device=device) * float(weight)
            total = d if total is None else total + d
    return total
