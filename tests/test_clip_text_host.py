"""CLIP text towers and prompt encoding without a GPU: the host rules of consistentid_amd/clip_text.py (config mapping,
refusals, the id check, the EOS pooling index), prompt_encode.py with fake encoders (diffusers 0.23 semantics), the
SDXL trigger-word variant on real CLIPTokenizers built offline, the component reader, and the new C exports' refusals."""
import json
import os

import pytest
import torch

from consistentid_amd import clip_text, loader, prompt_encode


# ----------------------------------------------------------------------------- an offline CLIPTokenizer
def _byte_alphabet():
    """GPT-2's byte -> unicode table (the base alphabet of CLIP's BPE vocabulary)"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return [chr(c) for c in cs]


MERGES = ("a n</w>", "m an</w>", "f a", "fa c", "fac e</w>")


def make_tokenizer_dir(folder, merges=MERGES) -> int:
    """vocab.json / merges.txt / tokenizer_config.json of a tiny CLIP BPE tokenizer (byte alphabet, its </w> forms, a few
    merges, then <|startoftext|> and <|endoftext|> as the two highest ids like CLIP's); returns the vocabulary size"""
    os.makedirs(folder, exist_ok=True)
    chars = _byte_alphabet()
    vocab = chars + [c + "</w>" for c in chars] + ["</w>"] + ["".join(m.split()) for m in merges]
    vocab += ["<|startoftext|>", "<|endoftext|>"]
    with open(os.path.join(folder, "vocab.json"), "w") as f:
        json.dump({t: i for i, t in enumerate(vocab)}, f)
    with open(os.path.join(folder, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n" + "".join(m + "\n" for m in merges))
    with open(os.path.join(folder, "tokenizer_config.json"), "w") as f:
        json.dump({"model_max_length": 77, "bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>",
                   "unk_token": "<|endoftext|>", "pad_token": "<|endoftext|>"}, f)
    return len(vocab)


def tiny_text_config(vocab_size, **kw):
    from transformers import CLIPTextConfig
    args = dict(vocab_size=vocab_size, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=64, eos_token_id=2, bos_token_id=0,
                pad_token_id=1)
    args.update(kw)
    return CLIPTextConfig(**args)


# ----------------------------------------------------------------------------- config, refusals, ids, pooling
def test_text_config_mapping_and_refusals():
    cfg = clip_text.text_config({"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12,
                                 "num_attention_heads": 12, "hidden_act": "quick_gelu", "eos_token_id": 2})
    assert (cfg.hidden_size, cfg.head_dim, cfg.num_hidden_layers, cfg.eos_token_id) == (768, 64, 12, 2)
    assert cfg.vocab_size == 49408 and cfg.max_position_embeddings == 77 and cfg.layer_norm_eps == 1e-5
    big = clip_text.text_config(tiny_text_config(49408, hidden_size=1280, num_attention_heads=20, hidden_act="gelu"))
    assert big.head_dim == 64 and big.hidden_act == "gelu"
    with pytest.raises(NotImplementedError, match="hidden_act"):
        clip_text.text_config({"hidden_size": 768, "num_attention_heads": 12, "hidden_act": "gelu_new"})
    with pytest.raises(NotImplementedError, match="64-wide"):
        clip_text.text_config({"hidden_size": 640, "num_attention_heads": 8})


def _cpu_engine(vocab=600, **kw):
    from transformers import CLIPTextModel
    cfg = tiny_text_config(vocab, **kw)
    torch.manual_seed(0)
    return clip_text.HipCLIPTextModel(CLIPTextModel(cfg).state_dict(), cfg, device="cpu")


def test_engine_refuses_before_any_launch():
    """argument refusals happen on the host, before anything reaches the device (the engine here is built on the CPU)"""
    eng = _cpu_engine(vocab=600)
    ids = torch.randint(0, 600, (2, 77))
    with pytest.raises(NotImplementedError, match="attention_mask"):
        eng(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(ValueError, match="sequence length 78"):
        eng(torch.zeros(1, 78, dtype=torch.long))
    bad = ids.clone()
    bad[1, 5] = 601                                        # e.g. a trigger token the table never got
    with pytest.raises(ValueError, match=r"token id 601 .*vocab size 600"):
        eng(bad)
    with pytest.raises(ValueError, match="token id -1"):
        clip_text.check_ids(torch.tensor([[0, -1]]), 600)
    clip_text.check_ids(torch.tensor([[0, 599]]), 600)


def test_engine_reads_both_key_layouts():
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    cfg = tiny_text_config(600)
    sd = CLIPTextModel(cfg).state_dict()
    prefixed = {("text_model." + k if not k.startswith("text_model.") else k): v for k, v in sd.items()}
    prefixed["text_model.embeddings.position_ids"] = torch.arange(77)[None]           # stray buffer of older checkpoints
    for d in (sd, prefixed):
        eng = clip_text.HipCLIPTextModel(d, cfg, device="cpu")
        assert not eng.with_projection and eng.n_layers == 2
    eng = clip_text.HipCLIPTextModel(CLIPTextModelWithProjection(cfg).state_dict(), cfg, device="cpu")
    assert eng.with_projection and tuple(eng.W["proj.w"].shape) == (64, 128)


@pytest.mark.parametrize("eos", [2, 599])
def test_pool_index_follows_transformers(eos):
    """pool_index picks the row transformers' pooler_output takes, for the legacy eos_token_id 2 (argmax of the ids) and a
    real EOS id, with rows holding added-token ids ABOVE the EOS id (the trigger tokens) and repeated EOS padding"""
    from transformers import CLIPTextModel
    cfg = tiny_text_config(610, eos_token_id=eos)
    torch.manual_seed(1)
    m = CLIPTextModel(cfg).eval()
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(3, 590, (4, 77), generator=g)
    ids[:, 0] = 598
    for b, (n, extra) in enumerate([(10, None), (30, 605), (76, None), (5, 609)]):
        ids[b, n] = 599
        ids[b, n + 1:] = 599                                   # EOS padding (SD1.5's tokenizer pads with <|endoftext|>)
        if extra is not None:
            ids[b, n // 2] = extra                             # added token id above the EOS id
    with torch.no_grad():
        out = m(ids)
    idx = clip_text.pool_index(ids, eos)
    want = out.last_hidden_state[torch.arange(4), idx]
    assert torch.equal(want, out.pooler_output)
    if eos == 2:
        assert idx.tolist() == [10, 15, 76, 2]                 # argmax: the added ids win where present
    else:
        assert idx.tolist() == [10, 30, 76, 5]


# ----------------------------------------------------------------------------- prompt encoding with fakes
class FakeTok:
    """ids from characters: row = [BOS, ord(c) % 50 + 3 ..., EOS, pad...]"""
    model_max_length = 8

    def __init__(self, tag=0):
        self.tag = tag
        self.calls = []

    def __call__(self, text, padding=None, max_length=None, truncation=False, return_tensors=None):
        texts = [text] if isinstance(text, str) else list(text)
        self.calls.append((tuple(texts), max_length))
        rows = []
        for t in texts:
            r = [1] + [ord(c) % 50 + 3 for c in t] + [2]
            r = r[:max_length] if truncation else r
            rows.append(r + [0] * (max_length - len(r)))

        class Out:
            input_ids = torch.tensor(rows)
        return Out


class FakeOut:
    def __init__(self, first, hidden_states):
        self.first, self.hidden_states = first, hidden_states

    def __getitem__(self, i):
        assert i == 0
        return self.first


class FakeEncoder:
    """[0] = ids (+ tag) broadcast over C channels; hidden_states[-2] = 10 x that; pooled ([0] of a projection tower) =
    row sums"""

    def __init__(self, C, tag=0.0, projection=False):
        self.C, self.tag, self.projection = C, tag, projection

    def __call__(self, ids, output_hidden_states=False):
        h = ids.float()[..., None].expand(*ids.shape, self.C) + self.tag
        hs = (h, 10 * h, h) if output_hidden_states else None
        return FakeOut(h.sum(1) if self.projection else h, hs)


def test_encode_prompt_semantics():
    tok, enc = FakeTok(), FakeEncoder(4)
    emb = lambda texts: enc(tok(texts, max_length=8, truncation=True).input_ids)[0].half()
    pos, neg = prompt_encode.encode_prompt(tok, enc, ["ab", "cde"], num_images_per_prompt=2, negative_prompt=["x", "y"])
    assert pos.dtype == torch.float16 and pos.shape == (4, 8, 4)
    assert torch.equal(pos, emb(["ab", "ab", "cde", "cde"])) and torch.equal(neg, emb(["x", "x", "y", "y"]))
    pos, neg = prompt_encode.encode_prompt(tok, enc, "ab")              # "" negative, one image
    assert tok.calls[-1] == (("",), 8)                                  # padded to the prompt's length
    assert torch.equal(neg, emb([""])) and torch.equal(pos, emb(["ab"]))
    pos, neg = prompt_encode.encode_prompt(tok, enc, "ab", do_classifier_free_guidance=False)
    assert neg is None
    cat = prompt_encode.encode_prompt_legacy(tok, enc, "ab", None, 3, True, "zz")
    assert torch.equal(cat, torch.cat([emb(["zz"] * 3), emb(["ab"] * 3)]))                  # cat([neg, pos])
    with pytest.raises(ValueError, match="batch size"):
        prompt_encode.encode_prompt(tok, enc, ["a", "b"], negative_prompt=["n"])
    with pytest.raises(TypeError):
        prompt_encode.encode_prompt(tok, enc, ["a", "b"], negative_prompt="n")
    pe, ne = torch.randn(2, 8, 4), torch.randn(2, 8, 4)                 # precomputed: no tower needed, repeat only
    pos, neg = prompt_encode.encode_prompt(None, None, None, prompt_embeds=pe, negative_prompt_embeds=ne,
                                           num_images_per_prompt=2)
    assert torch.equal(pos, pe.half().repeat_interleave(2, 0)) and torch.equal(neg, ne.half().repeat_interleave(2, 0))
    with pytest.raises(ValueError, match="batch size"):
        prompt_encode.encode_prompt(None, None, None, prompt_embeds=pe, negative_prompt_embeds=ne[:1])
    with pytest.raises(NotImplementedError):
        prompt_encode.encode_prompt(tok, enc, "a", lora_scale=0.5)
    with pytest.raises(NotImplementedError):
        prompt_encode.encode_prompt(tok, enc, "a", clip_skip=1)


def test_encode_prompt_sdxl_semantics():
    t1, t2 = FakeTok(), FakeTok()
    e1, e2 = FakeEncoder(3, tag=0.0), FakeEncoder(5, tag=0.5, projection=True)
    ids = lambda tok, texts: tok(texts, max_length=8, truncation=True).input_ids
    pe, ne, pp, npool = prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], ["ab", "c"], num_images_per_prompt=2)
    assert pe.shape == (4, 8, 8) and pp.shape == (4, 5)
    want = torch.cat([e1(ids(t1, ["ab", "c"]), True).hidden_states[-2], e2(ids(t2, ["ab", "c"]), True).hidden_states[-2]], -1)
    assert torch.equal(pe, want.half().repeat_interleave(2, 0))                     # [CLIP-L | bigG], prompt_2 = prompt
    assert torch.equal(pp, e2(ids(t2, ["ab", "c"]))[0].half().repeat_interleave(2, 0))     # pooled from tower 2
    assert torch.equal(ne, torch.zeros_like(pe)) and torch.equal(npool, torch.zeros_like(pp))   # force_zeros
    pe, ne, pp, npool = prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], "ab", prompt_2="zz",
                                                         force_zeros_for_empty_prompt=False)
    assert torch.equal(pe[..., 3:], e2(ids(t2, ["zz"]), True).hidden_states[-2].half())
    assert torch.equal(pe[..., :3], e1(ids(t1, ["ab"]), True).hidden_states[-2].half())
    assert torch.equal(ne[..., :3], e1(ids(t1, [""]), True).hidden_states[-2].half())       # "" negative without force_zeros
    assert torch.equal(npool, e2(ids(t2, [""]))[0].half())
    pe2, ne2, _, _ = prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], "ab", negative_prompt="q", negative_prompt_2="r")
    assert torch.equal(ne2[..., :3], e1(ids(t1, ["q"]), True).hidden_states[-2].half())
    assert torch.equal(ne2[..., 3:], e2(ids(t2, ["r"]), True).hidden_states[-2].half())
    with pytest.raises(ValueError, match="pooled"):
        prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], None, prompt_embeds=pe)
    with pytest.raises(ValueError, match="batch size"):
        prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], ["a", "b"], negative_prompt=["n"])
    with pytest.raises(NotImplementedError):
        prompt_encode.encode_prompt_sdxl([t1, t2], [e1, e2], "a", lora_scale=1.0)


def test_sdxl_trigger_word_variant_keeps_the_tokenizer2_quirk(tmp_path):
    from transformers import CLIPTokenizer
    from consistentid_amd.prompt_utils import encode_prompt_with_trigger_word
    make_tokenizer_dir(tmp_path / "t1")
    make_tokenizer_dir(tmp_path / "t2")
    t1 = CLIPTokenizer.from_pretrained(str(tmp_path / "t1"), local_files_only=True)
    t2 = CLIPTokenizer.from_pretrained(str(tmp_path / "t2"), local_files_only=True)
    for t in (t1, t2):
        t.add_tokens(["<|image|>"], special_tokens=True)
    t1.add_tokens(["<|facial|>"], special_tokens=True)                  # load_ConsistentID_model: tokenizer 1 only
    fid = t1.convert_tokens_to_ids("<|facial|>")
    masks = {"Face": 1, "Nose": 2}
    out = prompt_encode.encode_prompt_with_trigger_word_sdxl(t1, t2, "a man", "The face is round, nose small.", dict(masks))
    text_only, ids1, ids2, masks_align, fmask, fidx, fidx_mask = out
    assert text_only.startswith("a man; Detail:") and "<|facial|>" not in text_only
    assert fid not in ids1[0].tolist() and int(fmask.sum()) == 2 and fidx_mask[0, :2].all()
    assert ids1.shape == ids2.shape == (1, 77) and set(masks_align) == {"Face", "Nose"}
    # tokenizer 2 does not know <|facial|>: the marker stays in its ids as ordinary BPE pieces
    face = "a man; Detail:" + out[0][len("a man; Detail:"):]
    assert fid not in ids2[0].tolist() and not torch.equal(ids1, ids2)
    pieces = t2.encode("<|facial|>")[1:-1]
    assert len(pieces) > 1 and all(p < t2.vocab_size for p in pieces)
    row2 = ids2[0].tolist()
    assert any(row2[i:i + len(pieces)] == pieces for i in range(77)), (pieces, row2)
    n = len(t2.encode(text_only))            # ids2 is longer than the text-only prompt by the two split markers
    assert row2.index(t2.eos_token_id) == n - 1 + 2 * len(pieces)
    # the SD1.5 form differs only in its joint ("Detail:" without "; ")
    sd15 = encode_prompt_with_trigger_word(t1, "a man", "The face is round, nose small.", dict(masks))
    assert sd15[0].startswith("a manDetail:") and face.startswith("a man; Detail:")
    long = prompt_encode.encode_prompt_with_trigger_word_sdxl(t1, t2, "a man", "x" * 331, {})
    assert long[0] == "a man"                                           # captions over 330 characters are dropped


# ----------------------------------------------------------------------------- loader
def test_text_components_from_a_model_directory(tmp_path):
    from transformers import CLIPTextModel, CLIPTextModelWithProjection
    root = tmp_path / "base"
    V = make_tokenizer_dir(root / "tokenizer")
    make_tokenizer_dir(root / "tokenizer_2")
    cfg = tiny_text_config(V)
    torch.manual_seed(0)
    m1, m2 = CLIPTextModel(cfg), CLIPTextModelWithProjection(tiny_text_config(V, hidden_act="gelu"))
    m1.save_pretrained(str(root / "text_encoder"))
    m2.save_pretrained(str(root / "text_encoder_2"))
    c1, sd1 = loader.read_component(root / "text_encoder", loader.TEXT_WEIGHT_NAMES)
    assert clip_text.text_config(c1) == clip_text.text_config(cfg)
    ref = {k if k.startswith("text_model.") else "text_model." + k: v for k, v in m1.state_dict().items()}
    got = {k if k.startswith("text_model.") else "text_model." + k: v for k, v in sd1.items() if "position_ids" not in k}
    assert got.keys() == ref.keys() and all(torch.equal(got[k], ref[k]) for k in ref)
    with pytest.raises(FileNotFoundError):
        loader.read_component(root / "text_encoder")                    # diffusers' file names are not transformers'
    with open(root / "model_index.json", "w") as f:
        json.dump({"force_zeros_for_empty_prompt": False}, f)
    assert loader.read_force_zeros(root) is False and loader.read_force_zeros(tmp_path) is True
    te = loader.load_text_encoder(root / "text_encoder_2", device="cpu")
    assert te.with_projection and te.spec.hidden_act == "gelu"
    got = loader.read_text_components(root, device="cpu", given={"text_encoder": None, "tokenizer_2": "mine"})
    assert got["text_encoder"] is None and got["tokenizer_2"] == "mine"
    assert got["text_encoder_2"].with_projection and got["tokenizer"].model_max_length == 77
    assert loader.read_text_components(tmp_path, device="cpu") == {}     # no folders: nothing read


# ----------------------------------------------------------------------------- C exports
def test_new_c_exports_refuse_bad_arguments(lib):
    assert all(hasattr(lib, n) for n in ("cid_self_attn_causal_f16", "cid_quick_gelu_f16", "cid_text_embed_f16"))
    attn = lambda *a: lib.cid_self_attn_causal_f16(*a, None)
    assert attn(None, 16, 16, 16, 1, 128, 12, 64, 1536, 1536, 64, 768, 77) == -22
    assert b"null pointer" in lib.cid_last_error()
    assert attn(16, 16, 16, 16, 1, 128, 10, 80, 1600, 1600, 96, 800, 77) == -22
    assert b"head dim 80" in lib.cid_last_error()
    assert attn(16, 16, 16, 16, 1, 100, 12, 64, 1536, 1536, 64, 768, 77) == -22
    assert b"multiple of 64" in lib.cid_last_error()
    assert attn(16, 16, 16, 16, 1, 128, 12, 64, 1536, 1536, 64, 768, 129) == -22
    assert b"n_keys" in lib.cid_last_error()
    assert attn(16, 16, 16, 16, 1, 128, 12, 64, 1536, 1536, 64, 764, 77) == -22
    assert b"pitches" in lib.cid_last_error()
    assert lib.cid_quick_gelu_f16(None, 8, None) == -22
    assert lib.cid_quick_gelu_f16(16, 12, None) == -22 and b"multiple of 8" in lib.cid_last_error()
    assert lib.cid_text_embed_f16(None, 1, 77, 128, 16, 16, 16, 49408, 768, None) == -22
    assert lib.cid_text_embed_f16(16, 1, 77, 64, 16, 16, 16, 49408, 768, None) == -22        # Tp < T
    assert lib.cid_text_embed_f16(16, 1, 77, 128, 16, 16, 16, 49408, 770, None) == -22       # C % 8
    assert b"bad shape" in lib.cid_last_error()
