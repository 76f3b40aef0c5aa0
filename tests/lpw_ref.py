"""An independent restatement of the long-prompt-weighting scheme that consistentid_amd/prompt_weighting.py implements, for
tests/test_prompt_weighting_host.py and tests/test_gpu_long_context.py.

UNPINNED: diffusers' community pipeline ``lpw_stable_diffusion`` is not available here; both this file and the product
module restate its algorithm from the written rules.  They were written separately -- a token regular
expression and numpy here, a character scanner and torch there -- so that a slip in one shows against the other, but neither
is checked against the original file."""
import re

import numpy as np

TOKEN = re.compile(r"\\[()\[\]\\]|\(|\[|:[+-]?(?:\d+\.?\d*|\.\d+)\)|\)|\]|[^\\()\[\]:]+|:|\\")


def parse(text):
    out, rounds, squares = [], [], []

    def mul(start, f):
        for k in range(start, len(out)):
            out[k][1] *= f

    for tok in TOKEN.findall(text):
        if len(tok) == 2 and tok[0] == "\\":
            out.append([tok[1], 1.0])
        elif tok == "(":
            rounds.append(len(out))
        elif tok == "[":
            squares.append(len(out))
        elif len(tok) > 2 and tok[0] == ":" and tok[-1] == ")" and rounds:
            mul(rounds.pop(), float(tok[1:-1]))
        elif tok == ")" and rounds:
            mul(rounds.pop(), 1.1)
        elif tok == "]" and squares:
            mul(squares.pop(), 1 / 1.1)
        else:
            out.append([tok, 1.0])
    for start in rounds:
        mul(start, 1.1)
    for start in squares:
        mul(start, 1 / 1.1)
    if not out:
        return [["", 1.0]]
    k = 0
    while k + 1 < len(out):
        if out[k][1] == out[k + 1][1]:
            out[k][0] += out.pop(k + 1)[0]
        else:
            k += 1
    return out


def stream(tok, text, multiples):
    ids, ws = [], []
    for frag, w in parse(text):
        t = tok.encode(frag)[1:-1]
        ids += t
        ws += [w] * len(t)
    return ids[:75 * multiples], ws[:75 * multiples]


def multiple(streams, multiples):
    longest = max(len(s[0]) for s in streams)
    m = 1
    while 75 * m < longest and m < multiples:
        m += 1
    return m


def padded(tok, ids, ws, m):
    pad = tok.pad_token_id if getattr(tok, "pad_token_id", None) is not None else tok.eos_token_id
    fill = 75 * m - len(ids)
    return [tok.bos_token_id] + ids + [pad] * fill + [tok.eos_token_id], [1.0] + ws + [1.0] * fill + [1.0]


def chunks(tok, ids, m):
    rows = []
    for i in range(m):
        row = list(ids[75 * i:75 * i + 77])
        row[0], row[-1] = tok.bos_token_id, tok.eos_token_id
        rows.append(row)
    return rows


def weights_per_position(ws, m):
    out = []
    for i in range(m):
        out += [1.0] + list(ws[1 + 75 * i:1 + 75 * (i + 1)]) + [1.0]
    return out


def embed(tok, encoder, prompts, negatives, multiples):
    """encoder: [n, 77] int array -> [n, 77, Dc] float64 array.  -> (prompt embeds, negative embeds or None, m) in fp64"""
    texts = list(prompts) + list(negatives or [])
    streams = [stream(tok, t, multiples) for t in texts]
    m = multiple(streams, multiples)
    outs = []
    for ids, ws in streams:
        pi, pw = padded(tok, ids, ws, m)
        e = np.concatenate(list(np.asarray(encoder(np.asarray(chunks(tok, pi, m))), dtype=np.float64)), axis=0)      # [77 m, Dc]
        w = np.asarray(weights_per_position(pw, m), dtype=np.float64)
        before = e.mean()
        e = e * w[:, None]
        outs.append(e * (before / e.mean()))
    n = len(prompts)
    return np.stack(outs[:n]), (np.stack(outs[n:]) if negatives else None), m
