"""Host side of few-step sampling: LCMScheduler's schedule, config surface and multistep rows -- fed through the float64 model
of the kernel's row contract, against the stateful restatement of tests/lcm_ref.py --, the embed-row selectors of the
single pass, ``time_cond_proj_dim`` in the config reader and the guidance-scale embedding, and the argument checks of
cid_multistep_step_f16.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from lcm_ref import LCMRef, guidance_scale_embedding
from multistep_ref import RowEmulator

from consistentid_amd import scheduler as S

ROOT = Path(__file__).resolve().parents[1]
N_ELEM = 24
SD15_DDIM_JSON = {"_class_name": "DDIMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
                  "num_train_timesteps": 1000, "set_alpha_to_one": False, "steps_offset": 1, "trained_betas": None,
                  "clip_sample": False}


@pytest.mark.parametrize("n,want", [(1, [999]), (2, [999, 499]), (4, [999, 759, 519, 279]),
                                    (8, [999, 879, 759, 639, 519, 399, 279, 159]), (50, list(range(999, 0, -20)))])
def test_timesteps(n, want):
    sch, ref = S.LCMScheduler(), LCMRef()
    sch.set_timesteps(n)
    ref.set_timesteps(n)
    assert sch.timesteps.tolist() == want == ref.timesteps.tolist() and sch.timesteps.dtype == np.int64
    assert sch.num_inference_steps == n and len(want) == n


@pytest.mark.parametrize("n", [0, 51, -1])
def test_step_counts_outside_the_distilled_schedule_raise(n):
    with pytest.raises(ValueError, match="original_inference_steps"):
        S.LCMScheduler().set_timesteps(n)


def test_surface_and_config_round_trip():
    sch = S.LCMScheduler()
    assert sch.multistep and sch.init_noise_sigma == 1.0 and sch.order == 1 and sch.scale_model_input(3.0, 999) == 3.0
    assert isinstance(sch.config, S.SchedulerConfig)
    for key, value in dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50,
                           timestep_scaling=10.0, sigma_data=0.5, prediction_type="epsilon").items():
        assert sch.config[key] == value, key
    for pred in S.PREDICTION_TYPES:
        ddim = S.DDIMScheduler.from_config(SD15_DDIM_JSON, prediction_type=pred)
        lcm = S.LCMScheduler.from_config(ddim.config)
        back = S.DDIMScheduler.from_config(lcm.config)
        assert isinstance(lcm, S.LCMScheduler) and lcm.prediction_type == pred == back.prediction_type
        assert np.array_equal(lcm.alphas_cumprod, ddim.alphas_cumprod) and np.array_equal(back.alphas_cumprod, ddim.alphas_cumprod)
        assert (back.steps_offset, back.timestep_spacing) == (ddim.steps_offset, ddim.timestep_spacing)
        assert back.final_alpha_cumprod == ddim.final_alpha_cumprod
        for cls in (S.EulerDiscreteScheduler, S.PNDMScheduler, S.DPMSolverMultistepScheduler):
            assert cls.from_config(lcm.config).prediction_type == pred
    assert S.LCMScheduler.from_config(SD15_DDIM_JSON, original_inference_steps=100).original_inference_steps == 100
    ca, cn = sch.add_noise_coefficients(519)
    assert ca > 0 and cn > 0 and abs(ca * ca + cn * cn - 1.0) < 1e-12


@pytest.mark.parametrize("key,value", [("thresholding", True), ("clip_sample", True), ("use_karras_sigmas", True),
                                       ("beta_schedule", "linear"), ("prediction_type", "v_prediction")])
def test_raw_configs_with_what_is_not_built_are_refused(key, value):
    with pytest.raises(NotImplementedError):
        S.LCMScheduler.from_config({**SD15_DDIM_JSON, key: value})


def test_other_refusals():
    with pytest.raises(NotImplementedError, match="prediction_type"):
        S.LCMScheduler(prediction_type="sample")
    with pytest.raises(TypeError):
        S.LCMScheduler.from_config(SD15_DDIM_JSON, eta=1.0)
    with pytest.raises(ValueError):
        S.LCMScheduler(original_inference_steps=0)


def toy_model(x, t):
    """a fixed non-linear model output (one head: the single pass has no unconditional one)"""
    return 0.5 * np.cos(x - float(t) / 200.0) + 0.2 * x + 0.1 * np.tanh(0.7 * x)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint"])
@pytest.mark.parametrize("pred", S.PREDICTION_TYPES)
def test_rows_reproduce_the_stateful_sampler(pred, inpaint, first):
    """4 steps.  The two forms are algebraically equal: relative L2 <= 1e-9, the bound test_multistep_host.py holds the other
    samplers' rows to against their restatements.  Noise rows other than the ones a row names are NaN in the emulator."""
    n = 4
    rng = np.random.default_rng(10 * first + inpaint)
    x0, noises = rng.standard_normal(N_ELEM), rng.standard_normal((n - first - 1, N_ELEM))
    blend = None
    if inpaint:
        blend = ((rng.random(N_ELEM) > 0.5).astype(np.float64), rng.standard_normal(N_ELEM), rng.standard_normal(N_ELEM))
    sch, ref = S.LCMScheduler(prediction_type=pred), LCMRef(prediction_type=pred)
    sch.set_timesteps(n)
    ref.set_timesteps(n)
    rows = sch.coefficient_rows(inpaint, first, np.float64)
    assert rows.shape == (n, 16) and rows.dtype == np.float64 and np.isfinite(rows).all()
    emu, got, want = RowEmulator(N_ELEM, z=noises), x0.copy(), x0.copy()
    for i in range(first, n):
        e = toy_model(got, sch.timesteps[i])
        got = emu.step(rows[i], got, e, e, 7.5, *(blend or ()))
        k = i - first
        want = ref.step(toy_model(want, ref.timesteps[i]), i, want, noises[k] if k < len(noises) else None)
        if blend is not None:
            mask, init, noise = blend
            ini = ref.add_noise(init, noise, ref.timesteps[i + 1]) if i < n - 1 else init
            want = (1 - mask) * ini + mask * want
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert np.isfinite(got).all() and err <= 1e-9, f"LCM {pred} inpaint={inpaint} first={first}: rel_l2 {err:.3e}"
    rows32 = sch.coefficient_rows(inpaint, first, np.float32)
    assert rows32.dtype == np.float32 and np.array_equal(rows32, rows.astype(np.float32))
    packed = S.pack_step_rows(rows32)
    assert np.array_equal(packed[:, :12].view(np.float32), rows32[:, :12]) and np.all(rows[:, S.C_IN] == 1.0)
    assert np.array_equal(packed[:, 12:], rows[:, 12:].astype(np.int32))


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_rows_write_no_ring_slot_and_the_last_reads_no_noise(n):
    """every executed row but the last weighs noise row k = executed step; the last has c_z == 0 and names row 0 of a table it
    does not read; no row writes the ring, saves or restores; rows before ``first_step`` are idle"""
    sch = S.LCMScheduler()
    sch.set_timesteps(n)
    for first in range(n):
        rows = sch.coefficient_rows(True, first, np.float64)
        assert rows.shape == (n, 16)
        for i, row in enumerate(rows):
            assert int(row[12]) == -1 and int(row[13]) == 0 and row[15] == 0.0 and not row[4:8].any()
            if i < first:
                assert row.tolist() == S._idle_row()
            elif i == n - 1:
                assert row[S.C_Z] == 0.0 and int(row[14]) == 0 and (row[9], row[10]) == (1.0, 0.0)
                c_skip, c_out = sch.boundary_scalings(sch.timesteps[i])
                assert (row[2], row[3]) == (c_skip, c_out)
            else:
                assert row[S.C_Z] > 0.0 and int(row[14]) == i - first < n - first - 1
    # a last row whose noise table is all NaN still gives a finite sample in the emulator
    emu = RowEmulator(N_ELEM, z=np.full((1, N_ELEM), np.nan))
    x = np.linspace(-1, 1, N_ELEM)
    assert np.isfinite(emu.step(rows[-1], x, x, x, 1.0)).all()


@pytest.mark.parametrize("B", [1, 2])
def test_single_pass_selectors(B):
    """[n_ts, B]: text-only K/V rows [B, 2B) up to the merge step, augmented [2B, 3B) after it, counted from first_step; the
    ControlNets' selector and the CFG selector of the same arguments are what they were"""
    from consistentid_amd.denoise import step_rows
    for first, merge in ((0, 1), (1, 0), (0, 10)):
        rows = step_rows(4, first, merge, B, False, single_pass=True)
        cfg = step_rows(4, first, merge, B, False)
        assert tuple(rows.unet.shape) == (4, B) and rows.unet.dtype == torch.int32 and tuple(cfg.unet.shape) == (4, 2 * B)
        for i in range(4):
            merged = (i - first) > merge
            want = [b + (2 * B if merged else B) for b in range(B)]
            assert rows.unet[i].tolist() == want and bool(rows.merged[i]) == merged
            assert cfg.unet[i].tolist() == list(range(B)) + want
        assert torch.equal(rows.controlnet, cfg.controlnet) and torch.equal(rows.merged, cfg.merged)


def test_noise_refusals_and_the_pipelines_noise_path():
    """variance_noise without eta is LCM's own noise; every other class keeps refusing it, and LCM keeps refusing eta"""
    from types import SimpleNamespace
    from consistentid_amd import pipeline
    from consistentid_amd.denoise import check_eta
    z = torch.zeros(3, 1, 4, 8, 8)
    assert check_eta(S.LCMScheduler(), 0.0, z) == 0.0
    for cls in (S.DDIMScheduler, S.EulerDiscreteScheduler, S.PNDMScheduler, S.DPMSolverMultistepScheduler):
        with pytest.raises(ValueError, match="variance_noise without eta"):
            check_eta(cls(), 0.0, z)
    with pytest.raises(ValueError, match="only DDIMScheduler has an eta term"):
        check_eta(S.LCMScheduler(), 0.5, None)
    assert pipeline.LCMScheduler is S.LCMScheduler
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(SimpleNamespace(device="cpu"), use_graph=False)
    pipe.scheduler = S.LCMScheduler.from_config(pipe.scheduler.config)
    assert isinstance(pipe._engine.scheduler, S.LCMScheduler)
    lat = torch.zeros(1, 4, 8, 8)
    assert pipe._variance_noise(0.0, None, z, lat, 4) is z
    drawn = pipe._variance_noise(0.0, torch.Generator().manual_seed(1), None, lat, 4)
    assert tuple(drawn.shape) == (3, 1, 4, 8, 8) and drawn.dtype == torch.float16
    assert tuple(pipe._variance_noise(0.0, torch.Generator().manual_seed(1), None, lat, 4, first_step=1).shape) == (2, 1, 4, 8, 8)
    assert pipe._variance_noise(0.0, None, None, lat, 1) is None
    with pytest.raises(ValueError, match="eta"):
        pipe._variance_noise(1.0, None, None, lat, 4)


def test_read_scheduler_maps_the_class_name(tmp_path):
    import json
    from consistentid_amd import loader
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        {**SD15_DDIM_JSON, "_class_name": "LCMScheduler", "original_inference_steps": 50, "timestep_scaling": 10.0}))
    sch = loader.read_scheduler(tmp_path)
    assert isinstance(sch, S.LCMScheduler) and sch.original_inference_steps == 50


def test_unet_config_keeps_time_cond_proj_dim():
    from consistentid_amd import loader, unet_spec
    from test_loader import SD15_JSON
    assert loader.unet_config_from_diffusers(SD15_JSON).time_cond_proj_dim is None
    assert loader.unet_config_from_diffusers({**SD15_JSON, "time_cond_proj_dim": None}).time_cond_proj_dim is None
    cfg = loader.unet_config_from_diffusers({**SD15_JSON, "time_cond_proj_dim": 256})
    assert cfg.time_cond_proj_dim == 256 and cfg == unet_spec.sd15_config(time_cond_proj_dim=256)
    shapes = unet_spec.unet_param_shapes(cfg)
    assert shapes["time_embedding.cond_proj.weight"] == (320, 256) and "time_embedding.cond_proj.bias" not in shapes
    assert "time_embedding.cond_proj.weight" not in unet_spec.unet_param_shapes(unet_spec.sd15_config())


TINY_COND_DIM = 32      # the tiny model's time_cond_proj_dim in tests/test_gpu_lcm.py


@pytest.mark.parametrize("dim", [256, TINY_COND_DIM])
@pytest.mark.parametrize("w", [0.0, 0.5, 7.0])
def test_guidance_scale_embedding(w, dim):
    """fp32 against float64: the arguments reach 7000, where one fp32 ulp is 4.9e-4 -- and the product's exp / multiply add a
    few more: |error| <= 4e-3 of values in [-1, 1] (16 ulp of the largest argument)"""
    from consistentid_amd.unet import guidance_scale_embedding as product
    got = product(w, dim)
    want = guidance_scale_embedding(w, dim)
    assert tuple(got.shape) == (1, dim) and got.dtype == torch.float32
    assert np.abs(got[0].double().numpy() - want).max() <= 4e-3
    if w == 0.0:
        assert torch.equal(got[0], torch.cat([torch.zeros(dim // 2), torch.ones(dim // 2)]))


def test_symbol_is_declared_exported_and_bound(lib):
    from consistentid_amd import _lib, ops
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", (ROOT / "include" / "cid.h").read_text()))
    assert "cid_multistep_step_f16" in names and "cid_multistep_step_f16" in _lib.SIGNATURES
    assert hasattr(lib, "cid_multistep_step_f16") and callable(ops.multistep_step)
    assert lib.cid_version() >= 111


def test_single_pass_entry_refuses_bad_arguments(lib):
    """cid_multistep_step_f16 checks its arguments before it launches anything (no GPU needed): dummy non-null addresses"""
    f = lib.cid_multistep_step_f16
    p = 4096
    ok = dict(eps=p, lat=p, hist=p, saved=p, z=None, z_rows=0, row=p, mask=None, init=None, noise=None, B=1, per=16)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["eps"], a["lat"], a["hist"], a["saved"], a["z"], a["z_rows"], a["row"], a["mask"], a["init"], a["noise"],
                 a["B"], a["per"], None)
    for name in ("eps", "lat", "hist", "saved", "row"):
        assert call(**{name: None}) == -22 and b"null pointer" in lib.cid_last_error(), name
    assert call(mask=p) == -22 and b"mask/init/noise" in lib.cid_last_error()
    assert call(mask=p, init=p) == -22 and call(init=p, noise=p) == -22
    for B in (0, -1):
        assert call(B=B) == -22 and b"multiple of 8" in lib.cid_last_error()
    assert call(per=0) == -22 and call(per=-8) == -22
    assert call(B=1, per=12) == -22 and b"multiple of 8" in lib.cid_last_error()
    assert call(B=3, per=4) == -22
    assert call(z=p, z_rows=0) == -22 and call(z=None, z_rows=2) == -22 and call(z=p, z_rows=-1) == -22
    for name in ("eps", "lat", "hist", "saved", "row"):
        assert call(**{name: p + 8}) == -22 and b"16-byte aligned" in lib.cid_last_error(), name
    assert call(z=p + 2, z_rows=1) == -22 and b"16-byte aligned" in lib.cid_last_error()
    for name in ("mask", "init", "noise"):
        assert call(**{"mask": p, "init": p, "noise": p, name: p + 4}) == -22 and b"16-byte aligned" in lib.cid_last_error()


def test_lora_on_cond_proj_stays_refused():
    import dataclasses
    from consistentid_amd import lora, unet_spec
    cfg = dataclasses.replace(unet_spec.tiny_config("sd15"), time_cond_proj_dim=TINY_COND_DIM)
    key = "lora_unet_time_embedding_cond_proj"
    with pytest.raises(NotImplementedError, match=key):
        lora.parse_lora({key + ".lora_down.weight": torch.zeros(4, TINY_COND_DIM), key + ".lora_up.weight": torch.zeros(64, 4)}, cfg)
