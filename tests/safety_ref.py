"""Reference of the safety-checker tests: diffusers 0.23 ``StableDiffusionSafetyChecker.forward`` restated in plain
PyTorch on transformers' ``CLIPVisionModel`` (diffusers itself is not a dependency of the tests).  The module keeps
diffusers' parameter names and ``checkpoint_state_dict()`` gives them as a saved checker has them -- what
``HipSafetyChecker`` loads.  ``decide`` is the threshold loop, on numpy float32 scalars like the original
(``round(np.float32, 3) > 0``).
"""
import numpy as np
import torch
from torch import nn

N_CONCEPTS, N_SPECIAL = 17, 3


def cosine_distance(image_embeds, text_embeds):
    return torch.mm(nn.functional.normalize(image_embeds), nn.functional.normalize(text_embeds).t())


class SafetyCheckerRef(nn.Module):
    def __init__(self, vision_config, n_concepts: int = N_CONCEPTS, n_special: int = N_SPECIAL, seed: int = 0):
        from transformers import CLIPVisionModel
        super().__init__()
        torch.manual_seed(seed)
        self.vision_model = CLIPVisionModel(vision_config)
        P = vision_config.projection_dim
        self.visual_projection = nn.Linear(vision_config.hidden_size, P, bias=False)
        self.concept_embeds = nn.Parameter(torch.randn(n_concepts, P), requires_grad=False)
        self.special_care_embeds = nn.Parameter(torch.randn(n_special, P), requires_grad=False)
        self.concept_embeds_weights = nn.Parameter(torch.ones(n_concepts), requires_grad=False)
        self.special_care_embeds_weights = nn.Parameter(torch.ones(n_special), requires_grad=False)
        with torch.no_grad():                       # fp16-representable weights; LayerNorm gains / biases off their init
            for _, p in self.named_parameters():
                if p.ndim == 1 and p.shape[0] == vision_config.hidden_size:
                    p.add_(torch.randn_like(p) * 0.05)
                p.copy_(p.half().float())
        self.eval()

    def checkpoint_state_dict(self):
        """state_dict() under the key names of a saved StableDiffusionSafetyChecker: the tower at
        ``vision_model.vision_model.*`` (transformers releases whose CLIPVisionModel holds the transformer's modules
        directly give ``vision_model.*``; the files on disk keep the nested name)"""
        sd = self.state_dict()
        if any(k.startswith("vision_model.vision_model.") for k in sd):
            return dict(sd)
        return {("vision_model." + k if k.startswith("vision_model.") else k): v for k, v in sd.items()}

    @torch.no_grad()
    def image_embeds(self, clip_input):
        return self.visual_projection(self.vision_model(clip_input)[1])        # [1]: pooled_output

    @torch.no_grad()
    def cosines(self, clip_input):
        """[B, n_special + n_concepts]: special-care columns first (the order the loop walks them in)"""
        e = self.image_embeds(clip_input)
        return torch.cat([cosine_distance(e, self.special_care_embeds), cosine_distance(e, self.concept_embeds)], dim=1)


def decide(cos, thresholds, n_special: int):
    """The loop of the forward for every image.  cos [B, K] and thresholds [K] (special-care first) as float32 ->
    (scores float32 [B, K] = cos - threshold + adjustment, unrounded; hits bool [B, K]; flags [B])"""
    cos = np.asarray(cos, dtype=np.float32)
    thr = np.asarray(thresholds, dtype=np.float32)
    B, K = cos.shape
    scores, hits = np.zeros((B, K), np.float32), np.zeros((B, K), bool)
    for b in range(B):
        adjustment = np.float32(0.0)
        for k in range(K):
            s = cos[b, k] - thr[k] + adjustment            # float32 throughout (numpy 2 keeps Python floats weak)
            scores[b, k] = s
            hits[b, k] = round(s, 3) > 0
            if k < n_special and hits[b, k]:
                adjustment = np.float32(0.01)
    return scores, hits, hits[:, n_special:].any(axis=1)


def thresholds_for(cos0, raw_margins):
    """thresholds [K] that put ``cos0 - threshold`` (one image's cosines, before any adjustment) at ``raw_margins``"""
    return (np.asarray(cos0, np.float64) - np.asarray(raw_margins, np.float64)).astype(np.float32)


BOUNDARY = 0.0005          # round(s, 3) > 0 turns at 0.0005 (half to even: exactly 0.0005 rounds to 0.0)


def assert_clear_of_boundary(scores, margin: float = 0.003):
    """every score of every image sits at least ``margin`` from the rounding boundary, so that an fp16-engine cosine error
    far below it cannot turn a decision"""
    d = np.abs(np.asarray(scores, np.float64) - BOUNDARY)
    assert d.min() >= margin, f"a reference score lies {d.min():.5f} from the boundary (entry {np.unravel_index(d.argmin(), d.shape)})"


# raw margins (cos - threshold before the adjustment) of image 0 for the decision cases; s = special-care, c = concept.
# -0.015 stays below the boundary with the adjustment (-0.005), -0.005 crosses it (+0.005).
def decision_cases(K: int, n_special: int):
    lo, hi, deep = -0.005, 0.005, -0.015
    cases = {"no_hit": [lo] * K}
    m = [lo] * K
    m[n_special] = hi
    cases["concept_hit"] = m                                        # flagged
    if n_special >= 1:
        m = [deep] * K
        m[0] = hi
        cases["special_alone"] = m                                  # special hit, every later entry at -0.005: not flagged
        m = [deep] * K
        m[0], m[n_special] = hi, lo
        cases["special_lifts_concept"] = m                          # -0.005 + 0.01 -> flagged
    if n_special >= 3:
        m = [deep] * K
        m[0], m[1], m[2] = lo, hi, lo
        cases["special_1_lifts_2_not_0"] = m                        # hits exactly at 1 and 2: index 0 came before the hit
    return cases


def expected_hits0(name: str, K: int, n_special: int):
    """the hits of image 0 each case is built to give"""
    hit = {"no_hit": [], "concept_hit": [n_special], "special_alone": [0], "special_lifts_concept": [0, n_special],
           "special_1_lifts_2_not_0": [1, 2]}[name]
    return np.isin(np.arange(K), hit)


# ---------------------------------------------------------------------------------------------- cid_clip_head_f16 cases
# (B, C, P, K, n_special, ldx / C, seed): 9 of 64 lanes hold data; a row pitch wider than the row; the real ViT-L/14
# geometry (1024 -> 768, 3 + 17 rows); no concepts.  The seeds are fixed so that every reference score of every decision
# case clears the rounding boundary (test_safety_host.py checks that on the CPU).
HEAD_CASES = {"lanes9": (1, 72, 40, 3, 1, 1, 11), "pitch5": (3, 128, 64, 5, 2, 5, 12), "vit_l": (2, 1024, 768, 20, 3, 1, 13),
              "no_concepts": (3, 128, 64, 0, 0, 1, 14)}
HEAD_EPS = 1e-5


def head_inputs(name: str):
    """fp16 / fp32 CPU operands of one case: x [B, ldx], gamma, beta [C], w [P, C] fp16; concepts fp32 [K, P], normalised"""
    B, C, P, K, n_special, pitch, seed = HEAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, pitch * C, generator=g).half()
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).half()
    beta = (0.1 * torch.randn(C, generator=g)).half()
    w = (torch.randn(P, C, generator=g) / C ** 0.5).half()
    concepts = nn.functional.normalize(torch.randn(K, P, generator=g), dim=-1) if K else None
    return dict(B=B, C=C, P=P, K=K, n_special=n_special, ldx=pitch * C, x=x, gamma=gamma, beta=beta, w=w, concepts=concepts)


def head_ref64(case):
    """fp64 evaluation of the same fp16 inputs -> (e [B, P], cos [B, K] or None)"""
    C = case["C"]
    x = case["x"][:, :C].double()
    ln = nn.functional.layer_norm(x, (C,), case["gamma"].double(), case["beta"].double(), HEAD_EPS)
    e = ln @ case["w"].double().t()
    if not case["K"]:
        return e, None
    return e, (e / e.norm(dim=-1, keepdim=True).clamp_min(1e-12)) @ case["concepts"].double().t()


# ---------------------------------------------------------------------------------------------- checker end to end (toy)
SMALL = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=4, num_attention_heads=2, image_size=70,
             patch_size=14, projection_dim=64)            # the toy tower of test_gpu_idstack.py
_SMALL_REF = {}


def small_ref():
    """(SafetyCheckerRef on the toy tower, clip_input [2, 3, 70, 70] of fp16-representable values, its fp32 cosines
    [2, 20] as float32).  Computed once.  A random tower maps two images to nearby embeddings, so image 1's scores land
    within a few thousandths of image 0's: the input seed is one of the few for which all of them clear the boundary."""
    if not _SMALL_REF:
        from transformers import CLIPVisionConfig
        ref = SafetyCheckerRef(CLIPVisionConfig(**SMALL), seed=5)
        x = torch.randn(2, 3, 70, 70, generator=torch.Generator().manual_seed(30)).half().float()
        _SMALL_REF.update(ref=ref, x=x, cos=ref.cosines(x).numpy().astype(np.float32))
    return _SMALL_REF["ref"], _SMALL_REF["x"], _SMALL_REF["cos"]
