"""Long weighted prompts for the SD1.5-family pipelines: the emphasis syntax ``(word)``, ``[word]``, ``(word:1.3)`` and
prompts beyond CLIP's 77-token window, encoded in chunks of 75 tokens and concatenated along the token axis -- the
"long prompt weighting" scheme of diffusers' community pipeline ``lpw_stable_diffusion``.

UNPINNED: that community file is not vendored and was not available when this was written; the module restates the
algorithm from its description, like the schedulers restate diffusers' (scheduler.py).  The rules:

  * ``(`` opens a x1.1 scope, ``[`` a x1/1.1 scope; ``)`` / ``]`` close the innermost scope of their kind; ``:w)`` with a
    float w closes the innermost round scope with factor w instead of 1.1; ``\\(`` ``\\)`` ``\\[`` ``\\]`` ``\\\\`` are literals;
    unclosed scopes run to the end of the text; neighbouring fragments of equal weight are merged.
  * every fragment is tokenised without special tokens, every token carries its fragment's weight, the stream is cut at
    75 * max_embeddings_multiples tokens;
  * the effective multiple m (1 <= m <= the requested one) is the smallest that holds the longer of prompt and negative
    prompt; both are padded to 75 m + 2 ids ``[bos] + tokens + [pad] * ... + [eos]``;
  * chunk i = ids [75 i, 75 i + 77) with its first id set to bos and its last to eos, encoded by the text tower (``[0]``,
    after the final LayerNorm); the chunks are concatenated to [1, 77 m, Dc];
  * per-position weights: 1.0 at each chunk's bos / eos and on padding, the token weights in between;
    ``emb <- emb * w``, then every sample is rescaled by (mean before) / (mean after), means in fp32 over all rows and
    channels.

Not built: ``no_boseos_middle``, ``BREAK`` / ``AND`` / scheduled prompts, textual inversion, ``clip_skip``.
Host code: pure functions over a CLIPTokenizer-like object (``encode``, ``bos_token_id``, ``eos_token_id``,
``pad_token_id``) and a text-encoder callable (``encoder(ids)[0]``).
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

import torch

CHUNK = 75                  # tokens of a chunk between its bos and eos
WINDOW = CHUNK + 2          # CLIP's 77 positions
ROUND, SQUARE = 1.1, 1 / 1.1
MAX_TEXT_ROWS = 1024        # CID_XATTN_LONG_MAX_TXT (include/cid.h): most text rows the cross-attention kernels take

_FLOAT_CLOSE = re.compile(r":([+-]?(?:\d+\.?\d*|\.\d+))\)")
_ESCAPABLE = "()[]\\"


def parse_prompt_attention(text: str) -> List[List]:
    """``text`` -> [[fragment, weight], ...] by the scope rules in the module docstring.  A ``)`` / ``]`` / ``:w)`` without
    an open scope of its kind, and a backslash in front of any other character, are ordinary text."""
    res: List[List] = []
    round_open: List[int] = []        # index into res where each open scope starts
    square_open: List[int] = []

    def scale_from(start: int, factor: float):
        for frag in res[start:]:
            frag[1] *= factor

    def literal(s: str):
        res.append([s, 1.0])

    i, n = 0, len(text)
    run = ""                          # plain characters collected since the last control character

    def flush():
        nonlocal run
        if run:
            literal(run)
            run = ""

    while i < n:
        ch = text[i]
        if ch == "\\" and i + 1 < n and text[i + 1] in _ESCAPABLE:
            flush()
            literal(text[i + 1])
            i += 2
        elif ch == "(":
            flush()
            round_open.append(len(res))
            i += 1
        elif ch == "[":
            flush()
            square_open.append(len(res))
            i += 1
        elif ch == ")" and round_open:
            flush()
            scale_from(round_open.pop(), ROUND)
            i += 1
        elif ch == "]" and square_open:
            flush()
            scale_from(square_open.pop(), SQUARE)
            i += 1
        elif ch == ":" and round_open and (m := _FLOAT_CLOSE.match(text, i)):
            flush()
            scale_from(round_open.pop(), float(m.group(1)))
            i = m.end()
        else:
            run += ch
            i += 1
    flush()
    for start in round_open:
        scale_from(start, ROUND)
    for start in square_open:
        scale_from(start, SQUARE)
    if not res:
        return [["", 1.0]]
    merged = [res[0]]
    for frag, w in res[1:]:
        if w == merged[-1][1]:
            merged[-1][0] += frag
        else:
            merged.append([frag, w])
    return merged


def check_multiples(max_embeddings_multiples, cap_rows: int = MAX_TEXT_ROWS) -> int:
    """the keyword's range: an int from 1 to ``cap_rows // 77`` (``cap_rows``: most text rows the cross-attention kernels
    take)"""
    m = max_embeddings_multiples
    if isinstance(m, bool) or not isinstance(m, int):
        raise ValueError(f"max_embeddings_multiples must be an int, got {m!r}")
    top = cap_rows // WINDOW
    if not 1 <= m <= top:
        raise ValueError(f"max_embeddings_multiples = {m}: from 1 to {top} (the cross-attention kernels take at most "
                         f"{cap_rows} text rows)")
    return m


def tokens_with_weights(tokenizer, text: str, max_embeddings_multiples: int) -> Tuple[List[int], List[float]]:
    """the token stream of ``text`` without special tokens and each token's weight, cut at 75 * max_embeddings_multiples"""
    ids: List[int] = []
    weights: List[float] = []
    for frag, w in parse_prompt_attention(text):
        toks = list(tokenizer.encode(frag))[1:-1]
        ids += toks
        weights += [float(w)] * len(toks)
    cut = CHUNK * max_embeddings_multiples
    return ids[:cut], weights[:cut]


def effective_multiple(lengths: Sequence[int], max_embeddings_multiples: int) -> int:
    """smallest m >= 1 with 75 m >= the longest token stream, at most the requested multiple"""
    longest = max(list(lengths) + [0])
    return max(1, min(max_embeddings_multiples, -(-longest // CHUNK)))


def pad_ids_and_weights(tokenizer, ids: Sequence[int], weights: Sequence[float], m: int) -> Tuple[List[int], List[float]]:
    """``[bos] + ids + [pad] * ... + [eos]`` of 75 m + 2 entries and its weights (1.0 on bos, padding and eos)"""
    bos, eos = tokenizer.bos_token_id, tokenizer.eos_token_id
    pad = getattr(tokenizer, "pad_token_id", None)
    pad = eos if pad is None else pad
    n_pad = CHUNK * m - len(ids)
    assert n_pad >= 0, "pad_ids_and_weights: more tokens than 75 m"
    return [bos] + list(ids) + [pad] * n_pad + [eos], [1.0] + list(weights) + [1.0] * (n_pad + 1)


def chunk_ids(tokenizer, padded: Sequence[int], m: int) -> torch.Tensor:
    """[m, 77] int64: chunk i = padded[75 i : 75 i + 77] with bos in front and eos at the end"""
    rows = torch.tensor([list(padded[CHUNK * i:CHUNK * i + WINDOW]) for i in range(m)], dtype=torch.long)
    rows[:, 0], rows[:, -1] = tokenizer.bos_token_id, tokenizer.eos_token_id
    return rows


def position_weights(padded_weights: Sequence[float], m: int) -> torch.Tensor:
    """[77 m] fp64: per chunk, 1.0 at bos and eos and the padded stream's weights of its 75 tokens in between"""
    w = torch.ones(m, WINDOW, dtype=torch.float64)
    body = torch.tensor(list(padded_weights[1:1 + CHUNK * m]), dtype=torch.float64)
    w[:, 1:-1] = body.view(m, CHUNK)
    return w.reshape(-1)


def apply_weights(emb: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """emb [B, T, Dc], w [B, T]: emb * w, then each sample rescaled by (mean before) / (mean after); the means in fp32
    (fp64 for fp64 input) over all rows and channels.  Returned in emb's dtype."""
    acc = torch.float64 if emb.dtype == torch.float64 else torch.float32
    e = emb.to(acc)
    before = e.mean(dim=(-2, -1))
    e = e * w.to(device=e.device, dtype=acc).unsqueeze(-1)
    after = e.mean(dim=(-2, -1))
    return (e * (before / after)[:, None, None]).to(emb.dtype)


def encode_chunks(text_encoder, ids: torch.Tensor, device=None) -> torch.Tensor:
    """ids [m, 77] -> [1, 77 m, Dc]: the tower's ``[0]`` of every chunk, concatenated along the token axis"""
    out = text_encoder(ids if device is None else ids.to(device))[0]
    return out.reshape(1, -1, out.shape[-1])


def encode_weighted(tokenizer, text_encoder, prompts: Sequence[str], negatives: Optional[Sequence[str]],
                    max_embeddings_multiples: int, device=None):
    """-> (prompt_embeds [B, 77 m, Dc], negative_prompt_embeds [B, 77 m, Dc] or None, m): every text parsed, weighted and
    chunked with ONE effective multiple m for the whole call"""
    texts = list(prompts) + list(negatives or [])
    streams = [tokens_with_weights(tokenizer, t, max_embeddings_multiples) for t in texts]
    m = effective_multiple([len(s[0]) for s in streams], max_embeddings_multiples)
    embs = []
    for ids, weights in streams:
        padded, pw = pad_ids_and_weights(tokenizer, ids, weights, m)
        emb = encode_chunks(text_encoder, chunk_ids(tokenizer, padded, m), device)
        embs.append(apply_weights(emb, position_weights(pw, m)[None]))
    n = len(prompts)
    pos = torch.cat(embs[:n])
    neg = torch.cat(embs[n:]) if negatives else None
    return pos, neg, m


def empty_chunk_ids(tokenizer) -> torch.Tensor:
    """[1, 77]: ``[bos, pad x 75, eos]``, the chunk a prompt without further tokens continues with"""
    padded, _ = pad_ids_and_weights(tokenizer, [], [], 1)
    return chunk_ids(tokenizer, padded, 1)


def extend_with_empty_chunks(text_encoder, tokenizer, embeds: torch.Tensor, m: int, device=None) -> torch.Tensor:
    """embeds [B, 77 k, Dc] -> [B, 77 m, Dc]: the tower's output for the empty chunk appended m - k times (the pre-loop rule:
    the trigger-word prompt stays on the 77 window while the negative prompt spans m chunks)"""
    k = embeds.shape[1] // WINDOW
    if embeds.shape[1] != k * WINDOW or k > m:
        raise ValueError(f"extend_with_empty_chunks: {embeds.shape[1]} rows cannot be continued to {m} chunks of {WINDOW}")
    if k == m:
        return embeds
    ids = empty_chunk_ids(tokenizer)
    empty = text_encoder(ids if device is None else ids.to(device))[0]
    empty = empty.to(device=embeds.device, dtype=embeds.dtype).expand(embeds.shape[0], -1, -1)
    return torch.cat([embeds] + [empty] * (m - k), dim=1)
