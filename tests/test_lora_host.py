"""Community LoRA files on the host (consistentid_amd/lora.py): module names in every spelling, reading, validation,
the delta arithmetic, the text tower's merge (an engine built on the CPU) and the pipelines' adapter bookkeeping on a
stub engine.  No GPU."""
import types
import warnings

import pytest
import torch

from consistentid_amd import lora, unet_spec
from lora_cases import merged_state_dict, synthetic_lora, to_diffusers, to_kohya

CONFIGS = {"tiny": lambda: unet_spec.tiny_config("sd15"), "tinyxl": lambda: unet_spec.tiny_config("sdxl"),
           "sd15": unet_spec.sd15_config, "sdxl": unet_spec.sdxl_config}
TOWER = types.SimpleNamespace(num_hidden_layers=2, hidden_size=128, intermediate_size=256)


# --------------------------------------------------------------------------- names
@pytest.mark.parametrize("name", list(CONFIGS))
def test_unet_names_round_trip(name):
    cfg = CONFIGS[name]()
    modules = lora.unet_modules(cfg)
    per_block = len(lora.BLOCK_MODULES)
    downs, mid, ups = unet_spec.walk(cfg)
    tfm = [t for blk in downs + [mid] + ups for t in blk.attentions]
    assert len(modules) == sum(2 + per_block * t.n_layers for t in tfm)       # proj_in, proj_out and the blocks
    shapes = unet_spec.unet_param_shapes(cfg)
    for path, (o, i) in modules.items():
        assert shapes[path + ".weight"][:2] == (o, i)
    for sgm in ((False, True) if cfg.family == "sdxl" else (False,)):
        table = lora.unet_name_table(cfg, sgm=sgm)
        assert len(table) == len(modules) and set(table.values()) == set(modules)        # a bijection
        for kohya, path in table.items():
            assert "." not in kohya and kohya == lora.kohya_name(lora.sgm_path(cfg, path) if sgm else path)
            assert kohya.startswith(("input_blocks_", "middle_block_", "output_blocks_")) == sgm
    assert not set(lora.unet_other_modules(cfg)) & set(modules)
    assert "conv_in" in lora.unet_other_modules(cfg) and "down_blocks.0.resnets.0.time_emb_proj" in lora.unet_other_modules(cfg)


@pytest.mark.parametrize("layers", [12, 32])
def test_tower_names_round_trip(layers):
    modules = lora.tower_modules(layers)
    table = lora.tower_name_table(layers)
    assert len(modules) == 6 * layers == len(table) and set(table.values()) == set(modules)
    assert all(k == lora.kohya_name(p) and "." not in k for k, p in table.items())


def test_pinned_names():
    sgm = lora.unet_name_table(unet_spec.sdxl_config(), sgm=True)
    for kohya, path in (
            ("lora_unet_input_blocks_4_1_transformer_blocks_0_attn1_to_q", "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"),
            ("lora_unet_input_blocks_8_1_transformer_blocks_9_ff_net_2", "down_blocks.2.attentions.1.transformer_blocks.9.ff.net.2"),
            ("lora_unet_middle_block_1_proj_in", "mid_block.attentions.0.proj_in"),
            ("lora_unet_output_blocks_0_1_transformer_blocks_0_attn2_to_k", "up_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k"),
            ("lora_unet_output_blocks_5_1_proj_out", "up_blocks.1.attentions.2.proj_out")):
        assert sgm[kohya[len("lora_unet_"):]] == path
        assert "lora_unet_" + lora.kohya_name(lora.sgm_path(unet_spec.sdxl_config(), path)) == kohya
    assert lora.unet_name_table(unet_spec.sd15_config())["mid_block_attentions_0_proj_in"] == "mid_block.attentions.0.proj_in"
    assert lora.tower_name_table(12)["text_model_encoder_layers_11_mlp_fc2"] == "text_model.encoder.layers.11.mlp.fc2"
    flat = {"lora_te_text_model_encoder_layers_11_mlp_fc2.lora_down.weight": torch.zeros(4, 3072),
            "lora_te_text_model_encoder_layers_11_mlp_fc2.lora_up.weight": torch.zeros(768, 4),
            "lora_unet_mid_block_attentions_0_proj_in.lora_down.weight": torch.zeros(4, 1280, 1, 1),
            "lora_unet_mid_block_attentions_0_proj_in.lora_up.weight": torch.zeros(1280, 4, 1, 1)}
    clip_l = types.SimpleNamespace(num_hidden_layers=12, hidden_size=768, intermediate_size=3072)
    got = lora.parse_lora(flat, unet_spec.sd15_config(), {"text_encoder": clip_l})
    assert list(got["unet"]) == ["mid_block.attentions.0.proj_in"]
    assert list(got["text_encoder"]) == ["text_model.encoder.layers.11.mlp.fc2"]


# --------------------------------------------------------------------------- one content, every spelling
def _same(a, b):
    assert set(a) == set(b)                 # (a .safetensors file returns its keys sorted)
    for path in a:
        (d1, u1, a1), (d2, u2, a2) = a[path], b[path]
        assert torch.equal(d1, d2) and torch.equal(u1, u2) and a1 == a2, path


@pytest.mark.parametrize("name", ["tiny", "tinyxl"])
def test_one_content_every_spelling(name, tmp_path):
    from safetensors.torch import save_file
    cfg = CONFIGS[name]()
    shapes = lora.unet_modules(cfg)
    # with alphas: the kohya spellings (SD1.5 files shape proj_in / proj_out like the 1x1 convolutions they are)
    mods = synthetic_lora(shapes, 3, 0.01)
    assert {a for _, _, a in mods.values()} == {None, 2.0, 16.0}
    flat = to_kohya(mods, conv=name == "tiny")
    if name == "tiny":
        assert flat["lora_unet_mid_block_attentions_0_proj_in.lora_down.weight"].dim() == 4
    parsed = lora.parse_lora(flat, cfg)
    _same(parsed["unet"], mods)
    assert all(d.dim() == 2 and u.dim() == 2 for d, u, _ in parsed["unet"].values())
    assert not parsed["text_encoder"] and not parsed["text_encoder_2"]
    if name == "tinyxl":
        _same(lora.parse_lora(to_kohya(mods, name_of=lambda p: lora.sgm_path(cfg, p)), cfg)["unet"], mods)
    # without: kohya and the three diffusers spellings
    plain = synthetic_lora(shapes, 3, 0.01, alphas=False)
    for flat2 in (to_kohya(plain), to_diffusers(plain, style="peft"), to_diffusers(plain, style="lora"),
                  to_diffusers(plain, style="layer")):
        _same(lora.parse_lora(flat2, cfg)["unet"], plain)
    # the same file as a dict, .safetensors, .bin and a folder plus weight_name
    save_file({k: v.contiguous() for k, v in flat.items()}, str(tmp_path / "a.safetensors"))
    torch.save(flat, str(tmp_path / "a.bin"))
    for src, wn in ((flat, None), (tmp_path / "a.safetensors", None), (str(tmp_path / "a.bin"), None),
                    (tmp_path, "a.safetensors"), (str(tmp_path), "a.bin")):
        _same(lora.parse_lora(lora.read_lora(src, wn), cfg)["unet"], mods)


def test_tower_spellings():
    cfg = CONFIGS["tinyxl"]()
    mods = synthetic_lora(lora.tower_modules(2, 128, 256), 4, 0.01, alphas=False)
    towers = {"text_encoder": TOWER, "text_encoder_2": TOWER}
    for flat, target in ((to_kohya(mods, prefix="lora_te_"), "text_encoder"), (to_kohya(mods, prefix="lora_te1_"), "text_encoder"),
                         (to_kohya(mods, prefix="lora_te2_"), "text_encoder_2"),
                         (to_diffusers(mods, prefix="text_encoder."), "text_encoder"),
                         (to_diffusers(mods, prefix="text_encoder_2.", style="layer"), "text_encoder_2"),
                         (to_diffusers({p[len("text_model."):]: v for p, v in mods.items()}, prefix="text_encoder."), "text_encoder")):
        parsed = lora.parse_lora(flat, cfg, towers)
        _same(parsed[target], mods)
        assert sum(bool(v) for v in parsed.values()) == 1


# --------------------------------------------------------------------------- refusals
def _one(name="mid_block_attentions_0_proj_in", r=4, o=128, i=128, prefix="lora_unet_"):
    return {f"{prefix}{name}.lora_down.weight": torch.zeros(r, i), f"{prefix}{name}.lora_up.weight": torch.zeros(o, r)}


@pytest.mark.parametrize("key", [
    "lora_unet_mid_block_resnets_0_conv1", "lora_unet_down_blocks_0_downsamplers_0_conv", "lora_unet_conv_in", "lora_unet_conv_out",
    "lora_unet_up_blocks_1_resnets_0_conv_shortcut", "lora_unet_mid_block_resnets_0_time_emb_proj",
    "lora_unet_time_embedding_linear_1"])
def test_refuses_modules_without_lora_support(key):
    cfg = CONFIGS["tiny"]()
    flat = dict(_one(), **{key + ".lora_down.weight": torch.zeros(4, 8), key + ".lora_up.weight": torch.zeros(8, 4)})
    with pytest.raises(NotImplementedError, match=key):
        lora.parse_lora(flat, cfg)


def test_refuses_modules_without_lora_support_other_spellings():
    cfg = CONFIGS["tinyxl"]()
    for key in ("lora_unet_input_blocks_1_0_in_layers_2", "lora_unet_input_blocks_2_0_op", "lora_unet_time_embed_0",
                "lora_unet_label_emb_0_0", "lora_unet_out_2", "lora_unet_add_embedding_linear_1"):
        with pytest.raises(NotImplementedError, match=key):
            lora.parse_lora({key + ".lora_down.weight": torch.zeros(4, 8), key + ".lora_up.weight": torch.zeros(8, 4)}, cfg)
    with pytest.raises(NotImplementedError, match="mid_block.resnets.0.conv1"):
        lora.parse_lora({"unet.mid_block.resnets.0.conv1.lora_A.weight": torch.zeros(4, 8),
                         "unet.mid_block.resnets.0.conv1.lora_B.weight": torch.zeros(8, 4)}, cfg)
    many = {}
    for n in range(5):
        many.update(_one(f"mid_block_resnets_{n % 2}_conv{n}x"))        # five keys of no module at all -> ValueError
    with pytest.raises(ValueError) as e:
        lora.parse_lora(many, cfg)
    assert str(e.value).count("lora_unet_mid_block_resnets") == 3 and "7 more" in str(e.value)     # at most three keys named


@pytest.mark.parametrize("suffix", ["hada_w1_a", "lokr_w1", "lora_mid.weight", "dora_scale", "lora_magnitude_vector", "diff",
                                    "diff_b", "bias"])
def test_refuses_other_parametrisations(suffix):
    key = "lora_unet_mid_block_attentions_0_proj_in." + suffix
    with pytest.raises(NotImplementedError, match="another parametrisation") as e:
        lora.parse_lora(dict(_one(), **{key: torch.zeros(4)}), CONFIGS["tiny"]())
    assert key in str(e.value)


def test_refuses_bad_shapes_pairs_and_spellings():
    cfg = CONFIGS["tiny"]()
    lora.parse_lora(_one(), cfg)
    with pytest.raises(ValueError, match="mid_block.attentions.0.proj_in"):          # does not fit the module
        lora.parse_lora(_one(i=64), cfg)
    with pytest.raises(ValueError, match="mid_block.attentions.0.proj_in"):          # do not fit each other
        bad = _one()
        bad["lora_unet_mid_block_attentions_0_proj_in.lora_up.weight"] = torch.zeros(128, 8)
        lora.parse_lora(bad, cfg)
    for lost in (".lora_down.weight", ".lora_up.weight"):
        flat = {k: v for k, v in _one().items() if not k.endswith(lost)}
        flat["lora_unet_mid_block_attentions_0_proj_in.alpha"] = torch.tensor(4.0)
        with pytest.raises(ValueError, match="mid_block.attentions.0.proj_in.* without its"):
            lora.parse_lora(flat, cfg)
    for key in ("mid_block_attentions_0_proj_in.lora_down.weight", "lora_unet_mid_block_attentions_0_proj_in.weight",
                "lora_unet_mid_block_attentions_7_proj_in.lora_down.weight", "unet.mid_block.attentions.0.proj_in.lora_C.weight",
                "unet.mid_block.attentions.0.nothing.lora_A.weight"):
        with pytest.raises(ValueError, match="no known spelling") as e:
            lora.parse_lora(dict(_one(), **{key: torch.zeros(4, 128)}), cfg)
        assert key in str(e.value)
    with pytest.raises(ValueError, match="text_encoder.text_model.encoder.layers.1.mlp.fc1"):
        lora.parse_lora(_one("text_model_encoder_layers_1_mlp_fc1", o=128, i=128, prefix="lora_te_"), cfg, {"text_encoder": TOWER})
    with pytest.raises(ValueError, match="no known spelling"):       # layer 2 of a two-layer tower
        lora.parse_lora(_one("text_model_encoder_layers_2_mlp_fc1", o=256, prefix="lora_te_"), cfg, {"text_encoder": TOWER})


def test_missing_tower_is_skipped_with_one_warning():
    cfg = CONFIGS["tiny"]()
    flat = dict(_one(), **_one("text_model_encoder_layers_0_mlp_fc1", o=256, prefix="lora_te2_"),
                **_one("text_model_encoder_layers_1_mlp_fc1", o=256, prefix="lora_te2_"),
                **_one("text_model_encoder_layers_0_mlp_fc1", o=256, prefix="lora_te_"))
    with pytest.warns(UserWarning) as rec:
        parsed = lora.parse_lora(flat, cfg, {"text_encoder": TOWER, "text_encoder_2": None})
    assert [str(w.message) for w in rec if "lora_te2_" in str(w.message)] and len(rec) == 1
    assert list(parsed["unet"]) == ["mid_block.attentions.0.proj_in"] and len(parsed["text_encoder"]) == 1
    assert not parsed["text_encoder_2"]
    with pytest.warns(UserWarning) as rec:
        parsed = lora.parse_lora(flat, cfg)                              # no tower at all: two prefixes, two warnings
    assert len(rec) == 2 and list(parsed["unet"]) == ["mid_block.attentions.0.proj_in"]


def test_missing_file(tmp_path):
    with pytest.raises(FileNotFoundError):
        lora.read_lora(tmp_path / "nothing.safetensors")
    with pytest.raises(FileNotFoundError):
        lora.read_lora(tmp_path, "nothing.safetensors")
    with pytest.raises(FileNotFoundError):
        lora.read_lora("some-user/some-lora")                            # hub ids are not resolved


# --------------------------------------------------------------------------- the delta
@pytest.mark.parametrize("r,alpha", [(4, None), (4, 2.0), (16, 16.0), (16, 4.0), (48, 24.0), (48, None)])
def test_delta_against_float64(r, alpha):
    """(alpha / r) * up @ down in fp32; r = 48 is larger than the module's smaller dimension (32)"""
    g = torch.Generator().manual_seed(r)
    down, up = (torch.randn(r, 32, generator=g) * r ** -0.5).half(), (torch.randn(64, r, generator=g) * 0.05).half()
    want = (alpha / r if alpha is not None else 1.0) * (up.double() @ down.double())
    got = lora.delta(down, up, alpha)
    assert got.dtype == torch.float32 and got.shape == (64, 32)
    assert float((got.double() - want).abs().max()) <= 2 ** -22 * float(want.abs().max()) * r ** 0.5
    both = lora.merged_delta([({"m": (down, up, alpha)}, 0.5), ({"other": (down, up, alpha)}, 1.0), ({"m": (down, up, None)}, 2.0)], "m")
    want2 = 0.5 * want + 2.0 * (up.double() @ down.double())
    assert float((both.double() - want2).abs().max()) <= 2 ** -21 * float(want2.abs().max()) * r ** 0.5
    assert lora.merged_delta([({"other": (down, up, alpha)}, 1.0)], "m") is None


# --------------------------------------------------------------------------- the text tower's merge, on a CPU engine
def test_text_tower_set_lora_on_the_host():
    from transformers import CLIPTextModel
    from consistentid_amd import clip_text
    from test_clip_text_host import tiny_text_config
    cfg = tiny_text_config(600)
    torch.manual_seed(0)
    sd = {k[len("text_model."):] if k.startswith("text_model.") else k: v.half().float()
          for k, v in CLIPTextModel(cfg).state_dict().items()}
    eng = clip_text.HipCLIPTextModel(sd, cfg, device="cpu", keep_base=True)
    plain = clip_text.HipCLIPTextModel(sd, cfg, device="cpu")
    with pytest.raises(RuntimeError, match="keep_base"):
        plain.set_lora([])
    base = {k: v.clone() for k, v in eng.W.items()}
    ptrs = {k: v.data_ptr() for k, v in eng.W.items()}
    mods = synthetic_lora(lora.tower_modules(2, 128, 256), 5, 0.01)
    mods2 = synthetic_lora(lora.tower_modules(2, 128, 256), 6, 0.01, kinds=("mlp.fc1",))
    eng.set_lora([(mods, 0.7), (mods2, 0.5)])
    want = merged_state_dict(sd, [(mods, 0.7), (mods2, 0.5)], strip="text_model.")
    qs = (64 ** -0.5) * 1.4426950408889634
    changed = set()
    for i in range(2):
        p = f"encoder.layers.{i}."
        a = p + "self_attn."
        exp = {f"{i}.qkv.w": torch.cat([want[a + "q_proj.weight"].double() * qs, want[a + "k_proj.weight"].double(),
                                        want[a + "v_proj.weight"].double()]),
               f"{i}.o.w": want[a + "out_proj.weight"].double(), f"{i}.fc1.w": want[p + "mlp.fc1.weight"].double(),
               f"{i}.fc2.w": want[p + "mlp.fc2.weight"].double()}
        for k, v in exp.items():
            # one fp16 rounding of an fp32 sum: half an fp16 ulp (2^-11 relative) plus the fp32 noise of the sum
            err = (eng.W[k].double() - v).abs()
            assert bool((err <= v.abs() * 2 ** -11 + 2 ** -24 + 1e-6).all()), k
            assert not torch.equal(eng.W[k], base[k]), k
            changed.add(k)
    assert all(torch.equal(eng.W[k], base[k]) for k in base if k not in changed)          # biases, norms, embeddings
    assert {k: v.data_ptr() for k, v in eng.W.items()} == ptrs
    eng.set_lora([(mods, 0.0)])
    assert all(torch.equal(eng.W[k].view(torch.int16), base[k].view(torch.int16)) for k in base)
    eng.set_lora([(mods, 1.0)])
    eng.set_lora([])
    assert all(torch.equal(eng.W[k].view(torch.int16), base[k].view(torch.int16)) for k in base)
    assert all(not t.is_cuda for t in eng._base.values()) and len(eng._base) == 12


# --------------------------------------------------------------------------- adapter bookkeeping of the pipelines
class StubEngine:
    """stands where a HipUNet / HipCLIPTextModel goes: records the (adapter name, weight) lists ``set_lora`` is given"""

    def __init__(self, target, **attrs):
        self.target, self.calls, self.pipe, self.device = target, [], None, torch.device("cpu")
        self.__dict__.update(attrs)

    def require_base(self):
        pass

    def set_lora(self, entries):
        names = {id(parsed[self.target]): n for n, parsed in self.pipe._lora_adapters.items()}
        self.calls.append([(names[id(m)], w) for m, w in entries])


def _stub_pipeline(tower=True):
    from consistentid_amd import pipeline
    cfg = CONFIGS["tiny"]()
    unet = StubEngine("unet", config=cfg)
    te = StubEngine("text_encoder", spec=TOWER) if tower else None
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(unet, use_graph=False, text_encoder=te)
    for e in (unet, te):
        if e is not None:
            e.pipe = pipe
    return pipe, unet, te, cfg


def test_adapter_bookkeeping():
    pipe, unet, te, cfg = _stub_pipeline()
    shapes = lora.unet_modules(cfg)
    A = to_kohya(synthetic_lora(shapes, 1, 0.01, kinds=("proj_in",)))
    B = dict(to_kohya(synthetic_lora(shapes, 2, 0.01, kinds=("ff.net.2",))),
             **to_kohya(synthetic_lora(lora.tower_modules(2, 128, 256), 3, 0.01), prefix="lora_te_"))
    assert pipe.get_list_adapters() == [] and pipe.get_active_adapters() == []
    pipe.load_lora_weights(A)
    assert unet.calls[-1] == [("default_0", 1.0)] and te.calls == []              # nothing of A addresses the tower
    pipe.load_lora_weights(B, adapter_name="style", some_diffusers_keyword=True)
    assert unet.calls[-1] == [("default_0", 1.0), ("style", 1.0)] and te.calls[-1] == [("style", 1.0)]
    pipe.load_lora_weights(A)                                                    # the next free default name
    assert pipe.get_list_adapters() == ["default_0", "style", "default_1"] == pipe.get_active_adapters()
    with pytest.raises(ValueError, match="already loaded"):
        pipe.load_lora_weights(A, adapter_name="style")
    n_calls = len(unet.calls)
    with pytest.raises(NotImplementedError):
        pipe.load_lora_weights(dict(A, **_one("conv_in", o=64, i=36)), adapter_name="bad")
    assert len(unet.calls) == n_calls and "bad" not in pipe.get_list_adapters()
    # set_adapters: a string, a list, one float for all, a list of weights (None = 1.0); the order stays the load order
    pipe.set_adapters("style")
    assert unet.calls[-1] == [("style", 1.0)] == te.calls[-1] and pipe.get_active_adapters() == ["style"]
    pipe.set_adapters(["default_1", "default_0"], [0.25, None])
    assert unet.calls[-1] == [("default_0", 1.0), ("default_1", 0.25)] and te.calls[-1] == []
    pipe.set_adapters(["style", "default_0"], 0.5)
    assert unet.calls[-1] == [("default_0", 0.5), ("style", 0.5)] and te.calls[-1] == [("style", 0.5)]
    for names, weights in ((["style", "nobody"], None), (["style"], [1.0, 2.0]), (["style", "style"], None)):
        before = (len(unet.calls), pipe.get_active_adapters())
        with pytest.raises(ValueError):
            pipe.set_adapters(names, weights)
        assert before == (len(unet.calls), pipe.get_active_adapters())
    # fuse / unfuse: one multiplier on all active adapters, reset by unfuse_lora
    pipe.fuse_lora(0.5)
    assert unet.calls[-1] == [("default_0", 0.25), ("style", 0.25)] and te.calls[-1] == [("style", 0.25)]
    pipe.unfuse_lora()
    assert unet.calls[-1] == [("default_0", 0.5), ("style", 0.5)] and pipe.get_active_adapters() == ["default_0", "style"]
    pipe.fuse_lora()
    assert unet.calls[-1] == [("default_0", 0.5), ("style", 0.5)]
    # unload: every engine that held a LoRA is handed the empty list once, then left alone
    pipe.unload_lora_weights()
    assert unet.calls[-1] == [] == te.calls[-1] and pipe.get_list_adapters() == [] == pipe.get_active_adapters()
    n_unet, n_te = len(unet.calls), len(te.calls)
    pipe.unload_lora_weights()
    assert (len(unet.calls), len(te.calls)) == (n_unet, n_te)
    pipe.load_lora_weights(A)
    assert unet.calls[-1] == [("default_0", 1.0)] and len(te.calls) == n_te


def test_pipeline_without_the_tower_warns_and_loads_the_unet_part():
    pipe, unet, _, cfg = _stub_pipeline(tower=False)
    flat = dict(to_kohya(synthetic_lora(lora.unet_modules(cfg), 1, 0.01, kinds=("proj_out",))),
                **to_kohya(synthetic_lora(lora.tower_modules(2, 128, 256), 3, 0.01), prefix="lora_te_"))
    with pytest.warns(UserWarning, match="lora_te_"):
        pipe.load_lora_weights(flat)
    assert unet.calls == [[("default_0", 1.0)]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pipe.set_adapters("default_0", 0.5)
    assert not hasattr(pipe, "load_textual_inversion")          # textual inversion is not built


def test_every_pipeline_class_has_the_surface():
    from consistentid_amd import pipeline
    for cls in (pipeline.ConsistentIDStableDiffusionPipeline, pipeline.ConsistentIDStableDiffusionXLPipeline,
                pipeline.StableDiffusionInpaintConsistentIDPipeline, pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline):
        for m in ("load_lora_weights", "set_adapters", "fuse_lora", "unfuse_lora", "unload_lora_weights", "get_active_adapters",
                  "get_list_adapters"):
            assert callable(getattr(cls, m))
