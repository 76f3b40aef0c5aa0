"""Long weighted prompts on the host (consistentid_amd/prompt_weighting.py): the emphasis parser, token / weight streams,
padding, the effective multiple and the chunk ids on FakeTokenizer; the weighted, mean-restored embeddings of a deterministic
fp64 stub encoder against the independent restatement tests/lpw_ref.py; the keyword's range and its value 1 (today's path);
the pre-loop padding rule on stub components.

UNPINNED: diffusers' community pipeline ``lpw_stable_diffusion`` is not available here.  The product module and
tests/lpw_ref.py both restate its algorithm from the written rules; neither is checked against the original."""
import numpy as np
import pytest
import torch

import lpw_ref
from consistentid_amd import prompt_encode
from consistentid_amd import prompt_weighting as pw
from fake_tokenizer import FakeTokenizer

DC = 8


class ListTokenizer(FakeTokenizer):
    """FakeTokenizer that takes a list of texts as well (the negative prompt arrives as one on diffusers' path)"""

    def __call__(self, text, **kw):
        if isinstance(text, str):
            return super().__call__(text, **kw)
        rows = torch.cat([FakeTokenizer.__call__(self, t, **kw).input_ids for t in text])

        class Out:
            input_ids = rows
        return Out


class EosPadTokenizer(ListTokenizer):
    """CLIP-L's convention: padding is the end-of-text id"""
    pad_token_id = FakeTokenizer.eos_token_id


def stub_values(ids):
    """[n, T] ids -> [n, T, DC] fp64: depends on the id, the position and the channel; mean far from zero"""
    ids = np.asarray(ids, dtype=np.float64)
    t = np.arange(ids.shape[1], dtype=np.float64)[None, :, None]
    c = np.arange(DC, dtype=np.float64)[None, None, :]
    return np.sin(0.37 * ids[:, :, None] + 0.05 * t + 0.11 * c) + 0.5 + 0.01 * ids[:, :, None]


class StubEncoder:
    def __init__(self):
        self.calls = []

    def __call__(self, ids):
        self.calls.append(ids.clone())
        return (torch.from_numpy(stub_values(ids.cpu().numpy())),)


def words(n, start=0):
    return " ".join(f"w{start + k}" for k in range(n))


# ------------------------------------------------------------------------------------------------ parser
EXAMPLES = [
    ("an (important) word", [["an ", 1.0], ["important", 1.1], [" word", 1.0]]),
    ("(unbalanced", [["unbalanced", 1.1]]),
    ("\\(literal\\]", [["(literal]", 1.0]]),
    ("(unnecessary)(parens)", [["unnecessaryparens", 1.1]]),
    ("a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).",
     [["a ", 1.0], ["house", 1.573], [" ", 1.1], ["on", 1.0], [" a ", 1.1], ["hill", 0.55], [", sun, ", 1.1], ["sky", 1.4641],
      [".", 1.1]]),
    ("", [["", 1.0]]),
    ("[soft]", [["soft", 1 / 1.1]]),
    ("\\\\ stays", [["\\ stays", 1.0]]),
    ("stray ) and ] and :1.2)", [["stray ) and ] and :1.2)", 1.0]]),
    ("((a) b", [["a", 1.1 * 1.1], [" b", 1.1]]),
]


@pytest.mark.parametrize("text,want", EXAMPLES)
@pytest.mark.parametrize("parse", [pw.parse_prompt_attention, lpw_ref.parse], ids=["product", "restatement"])
def test_parser_examples(parse, text, want):
    got = parse(text)
    assert [f for f, _ in got] == [f for f, _ in want], got
    for (_, w), (_, x) in zip(got, want):
        assert abs(w - x) <= 1e-9, got


def test_parser_agrees_with_the_restatement_on_mixed_text():
    for text in ("((((ugly)))), [out of frame], (bad hands:1.3), extra [[limbs]] (", "a:b (c:d) e:.5) (f:.5)", "(x:1.)[y](z:-1)",
                 "back\\slash \\( (in\\)side)"):
        a, b = pw.parse_prompt_attention(text), lpw_ref.parse(text)
        assert [f for f, _ in a] == [f for f, _ in b], (a, b)
        assert all(abs(w - x) <= 1e-9 for (_, w), (_, x) in zip(a, b)), (a, b)


# ------------------------------------------------------------------------------------------------ streams, padding, chunks
def test_token_streams_and_weights():
    tok = FakeTokenizer()
    ids, ws = pw.tokens_with_weights(tok, "a (big:1.5) red [cat], sat", 3)
    assert ids == tok.encode("a big red cat, sat")[1:-1]               # the brackets are syntax, not tokens
    assert ws == pytest.approx([1.0, 1.5, 1.0, 1 / 1.1, 1.0, 1.0], abs=1e-12)
    long_text = words(100) + " (" + words(100, 100) + ")"
    ids, ws = pw.tokens_with_weights(tok, long_text, 2)
    assert len(ids) == len(ws) == 150 and ws[99] == 1.0 and ws[100] == pytest.approx(1.1)
    assert ids == tok.encode(words(200))[1:151]
    assert (ids, ws) == tuple(lpw_ref.stream(tok, long_text, 2))


def test_effective_multiple():
    for longest, asked, want in ((0, 3, 1), (1, 3, 1), (75, 3, 1), (76, 3, 2), (150, 3, 2), (151, 3, 3), (400, 3, 3), (151, 1, 1)):
        assert pw.effective_multiple([longest, 3], asked) == want, (longest, asked)
        assert lpw_ref.multiple([([0] * longest, []), ([0] * 3, [])], asked) == want
    assert pw.effective_multiple([10, 160], 4) == 3                    # the longer of prompt and negative prompt decides


@pytest.mark.parametrize("Tok", [FakeTokenizer, EosPadTokenizer])
def test_padding_and_chunk_ids(Tok):
    tok = Tok()
    ids, ws = pw.tokens_with_weights(tok, words(80) + " (" + words(10, 80) + ":2)", 3)
    assert len(ids) == 90
    m = pw.effective_multiple([len(ids)], 3)
    assert m == 2
    padded, pws = pw.pad_ids_and_weights(tok, ids, ws, m)
    assert len(padded) == len(pws) == 75 * m + 2
    assert padded[0] == tok.bos_token_id and padded[-1] == tok.eos_token_id and padded[1:91] == ids
    assert padded[91:-1] == [tok.pad_token_id] * 60
    assert pws[0] == 1.0 and pws[1:81] == [1.0] * 80 and pws[81:91] == [2.0] * 10 and pws[91:] == [1.0] * 61
    rows = pw.chunk_ids(tok, padded, m)
    assert rows.shape == (2, 77) and rows.dtype == torch.long
    assert rows[:, 0].tolist() == [tok.bos_token_id] * 2 and rows[:, -1].tolist() == [tok.eos_token_id] * 2
    assert rows[0, 1:76].tolist() == ids[:75] and rows[1, 1:16].tolist() == ids[75:] and rows[1, 16:76].tolist() == [tok.pad_token_id] * 60
    assert rows.tolist() == lpw_ref.chunks(tok, padded, m)
    w = pw.position_weights(pws, m)
    assert w.shape == (154,) and w[0] == w[76] == w[77] == w[153] == 1.0
    assert w[1:76].tolist() == [1.0] * 75 and w[78:83].tolist() == [1.0] * 5 and w[83:93].tolist() == [2.0] * 10
    assert w[93:].tolist() == [1.0] * 61
    assert w.tolist() == lpw_ref.weights_per_position(pws, m)
    assert pw.empty_chunk_ids(tok).tolist() == [[tok.bos_token_id] + [tok.pad_token_id] * 75 + [tok.eos_token_id]]


# ------------------------------------------------------------------------------------------------ embeddings
PROMPT = "a (((portrait:1.3)) of [a] woman, (" + words(90) + "), (sharp:0.7) focus"
NEGATIVE = "((((ugly)))), [out of frame], " + words(170, 500) + ", (bad hands:1.4)"


@pytest.mark.parametrize("Tok", [FakeTokenizer, EosPadTokenizer])
def test_weighted_embeddings_match_the_restatement(Tok):
    enc = StubEncoder()
    pos, neg, m = pw.encode_weighted(Tok(), enc, [PROMPT, "short (one)"], [NEGATIVE, ""], 3)
    rpos, rneg, rm = lpw_ref.embed(Tok(), stub_values, [PROMPT, "short (one)"], [NEGATIVE, ""], 3)
    assert m == rm == 3 and pos.dtype == neg.dtype == torch.float64
    assert tuple(pos.shape) == tuple(neg.shape) == (2, 231, DC)
    assert all(tuple(c.shape) == (3, 77) for c in enc.calls)
    for got, want, what in ((pos, rpos, "prompt"), (neg, rneg, "negative")):
        err = float(np.abs(got.numpy() - want).max())
        print(f"[lpw] {what}: max |diff| to the restatement {err:.3e}")
        assert np.allclose(got.numpy(), want, rtol=0, atol=1e-6), err
    # the weights did something, and the mean came back
    plain = torch.from_numpy(stub_values(np.asarray(enc.calls[0]))).reshape(231, DC)
    assert float((pos[0] - plain).abs().max()) > 1e-2
    assert float(pos[0].mean()) == pytest.approx(float(plain.mean()), rel=1e-12)


def test_multiple_follows_the_longer_text():
    enc = StubEncoder()
    pos, neg, m = pw.encode_weighted(FakeTokenizer(), enc, ["short"], [words(80)], 5)
    assert m == 2 and tuple(pos.shape) == tuple(neg.shape) == (1, 154, DC)
    pos, neg, m = pw.encode_weighted(FakeTokenizer(), enc, [words(400)], None, 3)
    assert m == 3 and neg is None and tuple(pos.shape) == (1, 231, DC)


def test_unweighted_short_prompt_at_3_equals_1_exactly():
    """pad id == eos id: the padded ids of the one chunk are the ids diffusers' path tokenises, the weights are all 1.0 and
    (mean before) / (mean after) is exactly 1"""
    prompt, negative = words(75), "blurry, low quality"
    one = prompt_encode.encode_prompt(EosPadTokenizer(), StubEncoder(), prompt, negative_prompt=negative)
    three = prompt_encode.encode_prompt(EosPadTokenizer(), StubEncoder(), prompt, negative_prompt=negative,
                                        max_embeddings_multiples=3)
    for a, b in zip(one, three):
        assert a.dtype == b.dtype == torch.float16 and tuple(a.shape) == tuple(b.shape) == (1, 77, DC)
        assert torch.equal(a, b)
    legacy = prompt_encode.encode_prompt_legacy(EosPadTokenizer(), StubEncoder(), prompt, negative_prompt=negative,
                                                max_embeddings_multiples=3)
    assert torch.equal(legacy, torch.cat([one[1], one[0]]))


def test_multiples_1_leaves_brackets_literal():
    tok, enc = FakeTokenizer(), StubEncoder()
    prompt_encode.encode_prompt(tok, enc, "a (big:1.5) cat", do_classifier_free_guidance=False)
    assert enc.calls[0][0].tolist() == tok("a (big:1.5) cat", padding="max_length", max_length=77, truncation=True).input_ids[0].tolist()
    assert tok.vocab["("] in enc.calls[0][0].tolist()
    enc3 = StubEncoder()
    prompt_encode.encode_prompt(tok, enc3, "a (big:1.5) cat", do_classifier_free_guidance=False, max_embeddings_multiples=2)
    assert tok.vocab["("] not in enc3.calls[0][0].tolist()
    # ... and a long prompt is cut at 77 as before
    enc1 = StubEncoder()
    pos, _ = prompt_encode.encode_prompt(tok, enc1, words(200), do_classifier_free_guidance=False)
    assert tuple(pos.shape) == (1, 77, DC)


def test_negative_follows_given_prompt_embeds():
    tok = FakeTokenizer()
    given = torch.randn(1, 154, DC).half()
    pos, neg = prompt_encode.encode_prompt(tok, StubEncoder(), None, negative_prompt="(bad)", prompt_embeds=given,
                                           max_embeddings_multiples=3)
    assert torch.equal(pos, given) and tuple(neg.shape) == (1, 154, DC)
    empty = torch.from_numpy(stub_values(pw.empty_chunk_ids(tok).numpy())).half()
    assert torch.equal(neg[:, 77:], empty)
    with pytest.raises(ValueError, match="chunks of 77"):
        prompt_encode.encode_prompt(tok, StubEncoder(), None, negative_prompt="x", prompt_embeds=torch.zeros(1, 100, DC),
                                    max_embeddings_multiples=3)


@pytest.mark.parametrize("bad", [0, -1, 14, 100, 2.0, None, True])
def test_keyword_range(bad):
    top = pw.MAX_TEXT_ROWS // 77
    assert top == 13
    with pytest.raises(ValueError, match="max_embeddings_multiples"):
        prompt_encode.encode_prompt(FakeTokenizer(), StubEncoder(), "x", max_embeddings_multiples=bad)
    with pytest.raises(ValueError, match="max_embeddings_multiples"):
        prompt_encode.encode_prompt_legacy(FakeTokenizer(), StubEncoder(), "x", max_embeddings_multiples=bad)
    with pytest.raises(ValueError, match="max_embeddings_multiples"):
        _pre_loop().prepare_id_prompt_embeds("x", _face(), None, bad)
    assert pw.check_multiples(top) == top and pw.check_multiples(1) == 1


def test_pipelines_take_the_keyword():
    import inspect
    from consistentid_amd import pipeline as P
    sd15 = (P.ConsistentIDStableDiffusionPipeline, P.StableDiffusionInpaintConsistentIDPipeline,
            P.StableDiffusionControlNetInpaintConsistentIDPipeline)
    for cls in sd15:
        for fn in (cls.__call__, cls.encode_prompt, cls._encode_prompt, cls.prepare_id_prompt_embeds):
            p = inspect.signature(fn).parameters
            assert "max_embeddings_multiples" in p and p["max_embeddings_multiples"].default == 1, (cls, fn)
    assert "max_embeddings_multiples" not in inspect.signature(P.ConsistentIDStableDiffusionXLPipeline.encode_prompt).parameters
    assert "prompt_embeds" in P.ConsistentIDStableDiffusionXLPipeline.encode_prompt.__doc__


# ------------------------------------------------------------------------------------------------ the pre-loop rule
def _face():
    from PIL import Image
    return Image.new("RGB", (64, 64), (120, 90, 80))


def _pre_loop():
    from consistentid_amd.pipeline import _IDPreLoop, _SD15PromptEncoding

    class Pre(_IDPreLoop, _SD15PromptEncoding):
        """the pre-loop with stub components: no GPU, no weights; the ID conditioner records what it is given"""

        def __init__(self):
            self.tokenizer, self.text_encoder, self.device = ListTokenizer(), StubEncoder(), torch.device("cpu")
            self.app = self.bise_net = self.image_encoder = object()
            self.id_conditioner = self.record
            self.seen = None

        def get_prepare_faceid(self, face_image):
            return torch.zeros(1, 512)

        def get_prepare_facemask(self, input_image_file):
            return {}, None

        def get_prepare_clip_image(self, input_image_file, key_parsing_mask_list, **kw):
            return torch.zeros(5, 3, 224, 224), torch.zeros(5, 512, 512)

        def _clip_hidden(self, pixel_values):
            return torch.zeros(pixel_values.shape[0], 4, DC)

        def record(self, **kw):
            self.seen = kw
            return "prompt_embeds"

    return Pre()


def test_pre_loop_padding_rule():
    prompt = "a (photo) of a man"                                      # brackets stay literal in the trigger-word prompt
    one = _pre_loop()
    assert one.prepare_id_prompt_embeds(prompt, _face(), "(bad:1.3)") == "prompt_embeds"
    assert tuple(one.seen["negative_embeds"].shape) == (1, 77, DC) and tuple(one.seen["facial_token_mask"].shape)[-1] == 77
    pre = _pre_loop()
    negative = "((((ugly)))), [out of frame], " + words(160) + ", (bad hands:1.4)"
    assert pre.prepare_id_prompt_embeds(prompt, [_face()], negative, 4) == "prompt_embeds"
    s = pre.seen
    m = 3                                                              # what the negative prompt needs, not the 4 asked for
    for k in ("text_embeds", "text_only_embeds", "negative_embeds"):
        assert tuple(s[k].shape) == (1, 77 * m, DC), (k, tuple(s[k].shape))
    assert tuple(s["facial_token_mask"].shape) == tuple(one.seen["facial_token_mask"].shape)[:-1] + (77 * m,)
    assert torch.equal(s["facial_token_mask"][..., :77], one.seen["facial_token_mask"]) and not s["facial_token_mask"][..., 77:].any()
    # the positive sets: the 77 rows of the plain call, then the empty chunk's output m - 1 times
    tok = pre.tokenizer
    empty = torch.from_numpy(stub_values(pw.empty_chunk_ids(tok).numpy()))
    for k in ("text_embeds", "text_only_embeds"):
        assert torch.equal(s[k][:, :77].double(), one.seen[k].double()), k
        for c in range(1, m):
            assert torch.equal(s[k][:, 77 * c:77 * (c + 1)].double(), empty.to(s[k].dtype).double()), (k, c)
    assert tok.vocab["("] in one.text_encoder.calls[0][0].tolist()      # the trigger-word prompt was tokenised with its brackets
    # the negative set: parsed, weighted, chunked
    want = lpw_ref.embed(tok, stub_values, [negative], None, 4)         # (the same tokenizer: ids go by first appearance)
    assert want[2] == m
    assert s["negative_embeds"].dtype == torch.float16
    assert np.allclose(s["negative_embeds"].double().numpy(), want[0], rtol=2.0 ** -10, atol=1e-6)
    # a negative prompt that fits one chunk keeps the call on 77 rows
    short = _pre_loop()
    short.prepare_id_prompt_embeds(prompt, _face(), "(bad:1.3)", 3)
    assert tuple(short.seen["text_embeds"].shape) == (1, 77, DC) and tuple(short.seen["facial_token_mask"].shape)[-1] == 77
