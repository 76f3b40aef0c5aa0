"""Prompt strings -> text embeddings with diffusers 0.23 semantics (the pre-loop calls of the reference):

  encode_prompt / _encode_prompt (SD1.5, inpaint, CN)   D: StableDiffusionPipeline.encode_prompt / _encode_prompt, called at
                                                        pipline_StableDiffusion_ConsistentID.py:469-475, :494-501
  encode_prompt_sdxl                                    D: StableDiffusionXLPipeline.encode_prompt, SDXL :552-565
  encode_prompt_with_trigger_word_sdxl                  pipline_StableDiffusionXL_ConsistentID.py:338-391

Pure functions over the tokenizer(s) and the text encoder callable(s): a tokenizer is anything CLIPTokenizer-like
(``__call__(text, padding=, max_length=, truncation=, return_tensors=).input_ids``, ``model_max_length``), a text encoder
anything called as ``encoder(ids)`` / ``encoder(ids, output_hidden_states=True)`` that returns ``[0]`` and
``.hidden_states`` like transformers' CLIP text models -- ``clip_text.HipCLIPTextModel`` on the GPU.  The pipelines wrap
these in thin methods (pipeline.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from .prompt_utils import (MAX_CAPTION_CHARS, prepare_image_token_idx, process_text_with_markers,
                           tokenize_and_mask_noun_phrases_ends)

PromptT = Union[str, List[str], None]


def _tokenize(tokenizer, text, max_length: Optional[int] = None) -> torch.Tensor:
    return tokenizer(text, padding="max_length", max_length=max_length or tokenizer.model_max_length, truncation=True,
                     return_tensors="pt").input_ids


def _batch_size(prompt, prompt_embeds) -> int:
    if isinstance(prompt, str):
        return 1
    if isinstance(prompt, list):
        return len(prompt)
    if prompt_embeds is None:
        raise ValueError("give either prompt or prompt_embeds")
    return prompt_embeds.shape[0]


def _repeat(t: torch.Tensor, n: int) -> torch.Tensor:
    """``t.repeat(1, n, ...).view(B * n, ...)``: every row n times in a row (diffusers' num_images_per_prompt)"""
    return t.repeat_interleave(n, dim=0)


def _refuse(lora_scale, clip_skip=None):
    if lora_scale is not None:
        raise NotImplementedError("lora_scale: text-encoder LoRA is not built")
    if clip_skip is not None:
        raise NotImplementedError("clip_skip is not built")


def _uncond_tokens(prompt, negative_prompt, batch_size: int) -> List[str]:
    """diffusers 0.23's rules for the unconditional text of the SD1.5 pipelines"""
    if negative_prompt is None:
        return [""] * batch_size
    if prompt is not None and type(prompt) is not type(negative_prompt):
        raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != "
                        f"{type(prompt)}.")
    if isinstance(negative_prompt, str):
        negative_prompt = [negative_prompt]
    if batch_size != len(negative_prompt):
        raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} "
                         f"has batch size {batch_size}. Please make sure that passed `negative_prompt` matches the batch "
                         "size of `prompt`.")
    return list(negative_prompt)


def encode_prompt(tokenizer, text_encoder, prompt: PromptT, device=None, num_images_per_prompt: int = 1,
                  do_classifier_free_guidance: bool = True, negative_prompt: PromptT = None,
                  prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                  lora_scale=None, clip_skip=None, max_embeddings_multiples: int = 1):
    """D: StableDiffusionPipeline.encode_prompt (0.23) -> (prompt_embeds, negative_prompt_embeds): the last hidden state
    (after final_layer_norm) of the padded, truncated prompt; the negative defaults to ""; each row repeated
    ``num_images_per_prompt`` times.  Without CFG the negative comes back as given (None by default).
    ``max_embeddings_multiples`` >= 2: long weighted prompts (prompt_weighting.py) -- the emphasis syntax is parsed and the
    texts are encoded in up to that many chunks of 75 tokens, [B, 77 m, Dc]; 1 is diffusers' path above (brackets are
    literal characters, truncation at 77)."""
    from .prompt_weighting import check_multiples
    _refuse(lora_scale, clip_skip)
    if check_multiples(max_embeddings_multiples) > 1:
        return _encode_prompt_weighted(tokenizer, text_encoder, prompt, device, num_images_per_prompt,
                                       do_classifier_free_guidance, negative_prompt, prompt_embeds, negative_prompt_embeds,
                                       max_embeddings_multiples)
    batch_size = _batch_size(prompt, prompt_embeds)
    if prompt_embeds is None:
        if text_encoder is None or tokenizer is None:
            raise ValueError("encoding a prompt string needs a tokenizer and a text_encoder")
        prompt_embeds = text_encoder(_tokenize(tokenizer, prompt))[0]
    prompt_embeds = prompt_embeds.to(device=device, dtype=torch.float16)
    seq_len = prompt_embeds.shape[1]
    prompt_embeds = _repeat(prompt_embeds, num_images_per_prompt)
    if do_classifier_free_guidance and negative_prompt_embeds is None:
        if text_encoder is None or tokenizer is None:
            raise ValueError("encoding the negative prompt needs a tokenizer and a text_encoder (or pass negative_prompt_embeds)")
        uncond = _uncond_tokens(prompt, negative_prompt, batch_size)
        negative_prompt_embeds = text_encoder(_tokenize(tokenizer, uncond, max_length=seq_len))[0]
    if do_classifier_free_guidance:
        if negative_prompt_embeds.shape[0] != batch_size:
            raise ValueError(f"negative_prompt_embeds has batch size {negative_prompt_embeds.shape[0]}, the prompt {batch_size}")
        negative_prompt_embeds = _repeat(negative_prompt_embeds.to(device=device, dtype=torch.float16), num_images_per_prompt)
    return prompt_embeds, negative_prompt_embeds


def _encode_prompt_weighted(tokenizer, text_encoder, prompt, device, num_images_per_prompt, do_classifier_free_guidance,
                            negative_prompt, prompt_embeds, negative_prompt_embeds, max_embeddings_multiples):
    """encode_prompt with ``max_embeddings_multiples`` >= 2: the texts that have to be encoded share one effective multiple;
    given embeddings of 77 m rows fix it"""
    from . import prompt_weighting as pw
    batch_size = _batch_size(prompt, prompt_embeds)
    need_neg = do_classifier_free_guidance and negative_prompt_embeds is None
    if (prompt_embeds is None or need_neg) and (text_encoder is None or tokenizer is None):
        raise ValueError("encoding a prompt string needs a tokenizer and a text_encoder")
    prompts = None if prompt_embeds is not None else ([prompt] if isinstance(prompt, str) else list(prompt))
    negatives = _uncond_tokens(prompt, negative_prompt, batch_size) if need_neg else None
    if prompts is not None:
        prompt_embeds, neg, _ = pw.encode_weighted(tokenizer, text_encoder, prompts, negatives, max_embeddings_multiples, device)
    elif negatives is not None:
        rows = prompt_embeds.shape[1]
        if rows % pw.WINDOW or rows // pw.WINDOW > max_embeddings_multiples:
            raise ValueError(f"prompt_embeds of {rows} rows with max_embeddings_multiples = {max_embeddings_multiples}: the "
                             f"negative prompt is encoded in chunks of {pw.WINDOW} rows, at most that many")
        neg, _, _ = pw.encode_weighted(tokenizer, text_encoder, negatives, None, rows // pw.WINDOW, device)
        neg = pw.extend_with_empty_chunks(text_encoder, tokenizer, neg, rows // pw.WINDOW, device)    # (a shorter negative prompt)
    if need_neg:
        negative_prompt_embeds = neg
    prompt_embeds = _repeat(prompt_embeds.to(device=device, dtype=torch.float16), num_images_per_prompt)
    if do_classifier_free_guidance:
        if negative_prompt_embeds.shape[0] != batch_size:
            raise ValueError(f"negative_prompt_embeds has batch size {negative_prompt_embeds.shape[0]}, the prompt {batch_size}")
        negative_prompt_embeds = _repeat(negative_prompt_embeds.to(device=device, dtype=torch.float16), num_images_per_prompt)
    return prompt_embeds, negative_prompt_embeds


def encode_prompt_legacy(tokenizer, text_encoder, prompt: PromptT, device=None, num_images_per_prompt: int = 1,
                         do_classifier_free_guidance: bool = True, negative_prompt: PromptT = None,
                         prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                         lora_scale=None, max_embeddings_multiples: int = 1):
    """D: ``_encode_prompt`` (deprecated form of 0.23, the one the reference calls): cat([negative, prompt])"""
    pos, neg = encode_prompt(tokenizer, text_encoder, prompt, device, num_images_per_prompt, do_classifier_free_guidance,
                             negative_prompt, prompt_embeds, negative_prompt_embeds, lora_scale,
                             max_embeddings_multiples=max_embeddings_multiples)
    return torch.cat([neg, pos]) if neg is not None else pos


def encode_prompt_sdxl(tokenizers: Sequence, text_encoders: Sequence, prompt: PromptT, prompt_2: PromptT = None,
                       device=None, num_images_per_prompt: int = 1, do_classifier_free_guidance: bool = True,
                       negative_prompt: PromptT = None, negative_prompt_2: PromptT = None,
                       prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                       pooled_prompt_embeds: Optional[torch.Tensor] = None,
                       negative_pooled_prompt_embeds: Optional[torch.Tensor] = None, lora_scale=None,
                       force_zeros_for_empty_prompt: bool = True):
    """D: StableDiffusionXLPipeline.encode_prompt (0.23) -> (prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds,
    negative_pooled_prompt_embeds).  ``tokenizers`` / ``text_encoders``: (CLIP-L, bigG), or the second alone.  Each tower
    gives its hidden_states[-2], concatenated [CLIP-L | bigG] on the last axis; the pooled embeds are the last tower's
    ``[0]`` (bigG's projected text_embeds).  ``prompt_2`` defaults to ``prompt``; a None negative gives zeros when
    ``force_zeros_for_empty_prompt``."""
    _refuse(lora_scale)
    prompt = [prompt] if isinstance(prompt, str) else prompt
    batch_size = len(prompt) if prompt is not None else _batch_size(None, prompt_embeds)
    pairs = [(t, e) for t, e in zip(tokenizers, text_encoders) if e is not None]

    def run(texts):
        hs, pooled = [], None
        for text, (tok, enc) in zip(texts, pairs):
            out = enc(_tokenize(tok, text), output_hidden_states=True)
            pooled = out[0]
            hs.append(out.hidden_states[-2])
        return torch.cat(hs, dim=-1), pooled

    if prompt_embeds is None:
        if not pairs:
            raise ValueError("encoding a prompt string needs the tokenizers and text encoders")
        prompt_2 = prompt_2 or prompt
        prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
        prompt_embeds, pooled_prompt_embeds = run([prompt, prompt_2])
    elif pooled_prompt_embeds is None:
        raise ValueError("prompt_embeds without pooled_prompt_embeds: pass both (they come from the same text encoder call)")
    zero_out = negative_prompt is None and force_zeros_for_empty_prompt
    if do_classifier_free_guidance and negative_prompt_embeds is None and zero_out:
        negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        negative_pooled_prompt_embeds = torch.zeros_like(pooled_prompt_embeds)
    elif do_classifier_free_guidance and negative_prompt_embeds is None:
        if not pairs:
            raise ValueError("encoding the negative prompt needs the tokenizers and text encoders")
        negative_prompt = negative_prompt or ""
        negative_prompt_2 = negative_prompt_2 or negative_prompt
        negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        negative_prompt_2 = batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str) else negative_prompt_2
        if prompt is not None and type(prompt) is not type(negative_prompt):
            raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != "
                            f"{type(prompt)}.")
        if batch_size != len(negative_prompt):
            raise ValueError(f"`negative_prompt` has batch size {len(negative_prompt)}, but `prompt` has batch size "
                             f"{batch_size}. Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
        negative_prompt_embeds, negative_pooled_prompt_embeds = run([negative_prompt, negative_prompt_2])
    elif do_classifier_free_guidance and negative_pooled_prompt_embeds is None:
        raise ValueError("negative_prompt_embeds without negative_pooled_prompt_embeds: pass both")
    h = lambda t: _repeat(t.to(device=device, dtype=torch.float16), num_images_per_prompt)
    prompt_embeds, pooled_prompt_embeds = h(prompt_embeds), h(pooled_prompt_embeds)
    if do_classifier_free_guidance:
        if negative_prompt_embeds.shape[0] != batch_size:
            raise ValueError(f"negative_prompt_embeds has batch size {negative_prompt_embeds.shape[0]}, the prompt {batch_size}")
        negative_prompt_embeds, negative_pooled_prompt_embeds = h(negative_prompt_embeds), h(negative_pooled_prompt_embeds)
    return prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds


def encode_prompt_with_trigger_word_sdxl(tokenizer, tokenizer_2, prompt: str, face_caption: str, key_parsing_mask_list,
                                         image_token: str = "<|image|>", facial_token: str = "<|facial|>",
                                         max_num_facials: int = 5, num_id_images: int = 1):
    """ref SDXL :338-391 -> (prompt_text_only, clean_input_id [1, T], clean_input_id2 [1, T], key_parsing_mask_list_align,
    facial_token_mask, facial_token_idx, facial_token_idx_mask).  Differs from the SD1.5 form (prompt_utils) in the
    "; Detail:" joint and in the second id row.

    Quirk kept on purpose: ``clean_input_id2`` is tokenised by ``tokenizer_2`` but with TOKENIZER 1's ``<|facial|>`` id
    (ref :380).  load_ConsistentID_model adds only ``<|image|>`` to tokenizer_2 (ref :176), so tokenizer_2 does not know
    ``<|facial|>``: it BPE-splits the marker into ordinary pieces, none of them equals that id, and the pieces stay in
    clean_input_id2 (the checkpoints were trained on this)."""
    caption_align, masks_align = process_text_with_markers(face_caption, key_parsing_mask_list)
    prompt_face = prompt + "; Detail:" + caption_align
    n_tok = len(tokenizer(prompt_face, max_length=tokenizer.model_max_length, padding="max_length", truncation=False,
                          return_tensors="pt").input_ids[0])
    if n_tok != 77:                                          # too long for one window: caption first, prompt after
        prompt_face = "; Detail:" + caption_align + " Caption:" + prompt
    if len(face_caption) > MAX_CAPTION_CHARS:
        prompt_face = prompt
    prompt_text_only = prompt_face.replace("<|facial|>", "").replace("<|image|>", "")
    facial_id = tokenizer.convert_tokens_to_ids(facial_token)
    clean_ids, image_mask, facial_mask = tokenize_and_mask_noun_phrases_ends(prompt_face, None, facial_id, tokenizer)
    _, _, facial_idx, facial_idx_mask = prepare_image_token_idx(image_mask, facial_mask, num_id_images, max_num_facials)
    clean_ids2, _, _ = tokenize_and_mask_noun_phrases_ends(prompt_face, None, facial_id, tokenizer_2)
    return prompt_text_only, clean_ids, clean_ids2, masks_align, facial_mask, facial_idx, facial_idx_mask
