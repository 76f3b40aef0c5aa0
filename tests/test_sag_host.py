"""Host side of self-attention guidance: every scheduler's ``sag_coefficients`` against the closed forms
and against its own noise model, the blur weights and the nearest-neighbour rule of the test-side restatement, ``check_sag``
and every refusal the pipelines and the engine make before a launch, and the argument checks of the five new entries.  No GPU."""
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sag_ref as R
from consistentid_amd import scheduler as S
from consistentid_amd import unet_spec as U

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("cid_attn_colmass_f16", "cid_sag_degrade_f16", "cid_cfg_sag_ddim_step_f16", "cid_cfg_sag_multistep_step_f16",
           "cid_sag_multistep_step_f16")
VP = (S.DDIMScheduler, S.PNDMScheduler, S.DPMSolverMultistepScheduler, S.LCMScheduler)


# ----------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("prediction", S.PREDICTION_TYPES)
@pytest.mark.parametrize("cls", VP, ids=lambda c: c.__name__)
def test_vp_coefficients_are_the_closed_forms(cls, prediction):
    sch = cls(prediction_type=prediction)
    sch.set_timesteps(4)
    for t in sch.timesteps:
        a = float(sch.alphas_cumprod[int(t)])
        sa, sb = a ** 0.5, (1.0 - a) ** 0.5
        want = (1 / sa, -sb / sa, 0.0, 1.0, sa, sb) if prediction == "epsilon" else (sa, -sb, sb, sa, sa, sb)
        assert np.allclose(sch.sag_coefficients(t), want, rtol=1e-15, atol=0)
        assert sch.sag_coefficients(t)[4:] == sch.add_noise_coefficients(t), "n_d, n_e are the scheduler's own add_noise"


@pytest.mark.parametrize("prediction", S.PREDICTION_TYPES)
def test_euler_coefficients_are_in_its_own_variables(prediction):
    sch = S.EulerDiscreteScheduler(prediction_type=prediction)
    sch.set_timesteps(4)
    for i, t in enumerate(sch.timesteps):
        sg = float(sch.sigmas[i])
        got = sch.sag_coefficients(t)
        if prediction == "epsilon":
            assert got == (1.0, -sg, 0.0, 1.0, 1.0, sg)
        else:       # diffusers: pred_original = -sigma v / sqrt(sigma^2 + 1) + x / (sigma^2 + 1); ehat = (x - pred_original) / sigma
            assert np.allclose(got, (1 / (sg * sg + 1), -sg / (sg * sg + 1) ** 0.5, sg / (sg * sg + 1), 1 / (sg * sg + 1) ** 0.5,
                                     1.0, sg), rtol=1e-15, atol=0)


@pytest.mark.parametrize("prediction", S.PREDICTION_TYPES)
@pytest.mark.parametrize("cls", VP + (S.EulerDiscreteScheduler,), ids=lambda c: c.__name__)
def test_noising_the_predicted_sample_again_gives_the_sample(cls, prediction):
    """add_noise(pred_x0(x, e), ehat(x, e)) == x to 1e-12 in float64, at every schedule entry"""
    sch = cls(prediction_type=prediction)
    sch.set_timesteps(5)
    g = np.random.default_rng(3)
    x, e = g.standard_normal(64), g.standard_normal(64)
    for t in sch.timesteps:
        p_x, p_e, q_x, q_e, n_d, n_e = sch.sag_coefficients(t)
        back = n_d * (p_x * x + p_e * e) + n_e * (q_x * x + q_e * e)
        assert np.abs(back - x).max() <= 1e-12 * max(1.0, n_e), (cls.__name__, t)


def test_the_table_has_a_row_per_evaluation():
    """PNDM's timestep list repeats its second entry: each of the two evaluations there has its own row; two zero words pad
    a row to 32 bytes"""
    sch = S.PNDMScheduler()
    sch.set_timesteps(4)
    tab = S.sag_coefficient_table(sch)
    assert tab.dtype == np.float32 and tab.shape == (5, 8) and (tab[:, 6:] == 0).all()
    assert sch.timesteps[1] == sch.timesteps[2] and (tab[1] == tab[2]).all() and not (tab[0] == tab[1]).all()
    for cls in VP + (S.EulerDiscreteScheduler,):
        sch = cls()
        sch.set_timesteps(3)
        assert S.sag_coefficient_table(sch).shape == (len(sch.timesteps), 8)
    zero = S.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    zero.set_timesteps(4)
    with pytest.raises(ValueError, match="not finite"):          # epsilon prediction where alphas_cumprod is 0
        S.sag_coefficient_table(zero)
    with pytest.raises(ValueError, match="not finite"):          # ... and at the source, for a direct caller
        zero.sag_coefficients(zero.timesteps[0])


def test_reference_noise_model_agrees_with_the_coefficients():
    """sag_ref reads the noise model off add_noise / scale_model_input of the REFERENCE schedulers and knows no table: its
    predictions are the product's coefficients, for both samplers' variables and both prediction types"""
    from oracle import ddim
    from vpred_ref import DDIMRef, EulerRef
    g = torch.Generator().manual_seed(5)
    x, out = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64), torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)
    for prod, ref, prediction in ((S.DDIMScheduler(), ddim.DDIMScheduler(), "epsilon"), (S.EulerDiscreteScheduler(), ddim.EulerDiscreteScheduler(), "epsilon"),
                                  (S.DDIMScheduler(prediction_type="v_prediction"), DDIMRef(prediction_type="v_prediction"), "v_prediction"),
                                  (S.EulerDiscreteScheduler(prediction_type="v_prediction"), EulerRef(prediction_type="v_prediction"), "v_prediction")):
        prod.set_timesteps(4)
        ref.set_timesteps(4)
        for tp, tr in zip(prod.timesteps, ref.timesteps):
            p_x, p_e, q_x, q_e, n_d, n_e = prod.sag_coefficients(tp)
            nd, ne, c_in = R.noise_model(ref, tr, x)
            assert abs(nd - n_d) <= 1e-6 * n_d and abs(ne - n_e) <= 1e-6 * n_e
            x0, ehat = R.predictions(x, out, nd, ne, prediction)
            assert torch.allclose(x0, p_x * x + p_e * out, rtol=1e-5, atol=1e-5) and torch.allclose(ehat, q_x * x + q_e * out, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------------------------------------- blur and mask
def test_blur_weights_and_fixed_point():
    w = R.blur_weights()
    assert w.shape == (9,) and abs(float(w.sum()) - 1.0) <= 1e-15 and torch.equal(w, w.flip(0))
    assert torch.allclose(w / w[4], torch.exp(-0.5 * (torch.arange(9, dtype=torch.float64) - 4) ** 2), rtol=1e-15, atol=0)
    const = torch.full((2, 3, 7, 5), 0.75, dtype=torch.float64)
    assert (R.blur(const) - const).abs().max() <= 1e-15, "a constant image is a fixed point (reflect padding keeps it constant)"
    ramp = torch.arange(40, dtype=torch.float64).reshape(1, 1, 5, 8)
    out = R.blur(ramp)
    assert tuple(out.shape) == (1, 1, 5, 8)
    # separable: rows, then columns, each against the reflected neighbours
    rows = torch.stack([sum(w[k] * ramp[0, 0, :, abs(x + k - 4) if x + k - 4 < 8 else 14 - (x + k - 4)] for k in range(9)) for x in range(8)], 1)
    both = torch.stack([sum(w[k] * rows[abs(y + k - 4) if y + k - 4 < 5 else 8 - (y + k - 4)] for k in range(9)) for y in range(5)], 0)
    assert torch.allclose(out[0, 0], both, rtol=1e-13, atol=1e-13)


def test_nearest_neighbour_rule():
    """source index floor(dst * in / out): 8 -> 64 repeats each cell eight times, 12 -> 96 likewise, and a ratio that is no
    integer (3 -> 8) follows the floor"""
    assert R.nearest_index(64, 8).tolist() == [i // 8 for i in range(64)]
    assert R.nearest_index(96, 12).tolist() == [i // 8 for i in range(96)]
    assert R.nearest_index(8, 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2]
    assert R.nearest_index(7, 3).tolist() == [(i * 3) // 7 for i in range(7)]
    mask = torch.tensor([[[True, False], [False, True]]])
    up = R.upsample_mask(mask, 4, 6)
    assert up[0, :2, :3].all() and not up[0, :2, 3:].any() and not up[0, 2:, :3].any() and up[0, 2:, 3:].all()
    mass = torch.tensor([[1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))]])
    assert (mass > 1.0).tolist() == [[False, True]], "the threshold is strict"


# ----------------------------------------------------------------------------------------------------------- keyword and refusals
class _StubUNet(SimpleNamespace):
    """what the pipelines and the engine touch of a UNet before the first launch"""

    def __init__(self):
        super().__init__(device="cpu", config=U.tiny_config("sd15"), pag_layers=(), enabled=[])

    def enable_pag(self, layers=U.PAG_DEFAULT_LAYERS):
        self.enabled.append(layers)
        self.pag_layers = tuple(U.pag_blocks(self.config, layers))


def _pipes():
    from consistentid_amd import pipeline
    return {"sd15": pipeline.ConsistentIDStableDiffusionPipeline, "sdxl": pipeline.ConsistentIDStableDiffusionXLPipeline,
            "inpaint": pipeline.StableDiffusionInpaintConsistentIDPipeline,
            "controlnet": pipeline.StableDiffusionControlNetInpaintConsistentIDPipeline}


def test_check_sag():
    from consistentid_amd.denoise import check_sag
    assert check_sag(0) == 0.0 and check_sag(0.75) == 0.75 and check_sag(np.float32(1.5)) == 1.5
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="sag_scale"):
            check_sag(bad)


def test_signatures():
    from consistentid_amd.denoise import DenoiseEngine
    from consistentid_amd.unet import HipUNet
    for name, cls in _pipes().items():
        assert inspect.signature(cls.__call__).parameters["sag_scale"].default == 0.0, name
    assert inspect.signature(DenoiseEngine.run).parameters["sag_scale"].default == 0.0
    assert inspect.signature(HipUNet.forward_tokens).parameters["sag"].default is None
    assert isinstance(DenoiseEngine.sag_mass, property)
    from consistentid_amd.pipeline import _BasePipeline
    assert isinstance(_BasePipeline.sag_mass, property)
    assert _pipes()["sd15"](_StubUNet(), use_graph=False).sag_mass is None


@pytest.mark.parametrize("name", ["sd15", "sdxl", "inpaint", "controlnet"])
def test_pipelines_validate_and_refuse_before_anything_runs(name):
    """ValueError for a negative or non-finite scale; NotImplementedError with pag_scale, with guidance_rescale and with
    ControlNet residuals -- all before the pre-loop, so the stub UNet and the missing inputs are never reached"""
    pipe = _pipes()[name](_StubUNet(), use_graph=False)
    for bad in (-0.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="sag_scale"):
            pipe(sag_scale=bad)
    with pytest.raises(NotImplementedError, match="pag_scale"):
        pipe(sag_scale=1.0, pag_scale=3.0) if name != "controlnet" else pipe._check_pag(3.0, 0.0, 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="guidance_rescale" if name != "controlnet" else "SAG with ControlNet residuals"):
        pipe(sag_scale=1.0, guidance_rescale=0.7)
    if name == "controlnet":
        with pytest.raises(NotImplementedError, match="SAG with ControlNet residuals"):
            pipe(sag_scale=1.0)
    if name == "inpaint":
        with pytest.raises(NotImplementedError, match="SAG with ControlNet residuals"):
            pipe(sag_scale=1.0, down_block_res_samples=[torch.zeros(1)], mid_block_res_sample=torch.zeros(1))
    assert pipe.unet.enabled == [], "a refused call must not change the UNet"


def test_scale_zero_adds_nothing_to_the_engine_call():
    """sag_scale == 0 yields the keywords, and so the step_path, of the call without it; > 0 reaches the engine alone"""
    pipe = _pipes()["sd15"](_StubUNet(), use_graph=False)
    assert pipe._check_pag(0.0, 0.0, 0.0, 0.0) == pipe._check_pag(0.0, 0.0) == dict(pag_scale=0.0, pag_adaptive_scale=0.0)
    assert pipe._check_pag(0.0, 0.0, 0.0, 0.75) == dict(sag_scale=0.75)
    assert pipe.unet.enabled == []


def test_engine_refuses_before_any_launch():
    """DenoiseEngine.run itself: the three combinations, named, before it touches its UNet's device -- the stub has none"""
    from consistentid_amd.denoise import DenoiseEngine
    unet = _StubUNet()
    eng = DenoiseEngine(unet, S.DDIMScheduler(), use_graph=False)
    lat, e = torch.zeros(1, 4, 8, 8), torch.zeros(1, 81, 128)
    kw = dict(num_inference_steps=4, guidance_scale=5.0, start_merge_step=1)
    with pytest.raises(NotImplementedError, match="pag_scale"):
        eng.run(lat, e, e, e, sag_scale=1.0, pag_scale=3.0, **kw)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        eng.run(lat, e, e, e, sag_scale=1.0, guidance_rescale=0.7, **kw)
    for extra in (dict(controlnet=object()), dict(down_residuals=[lat], mid_residual=lat)):
        with pytest.raises(NotImplementedError, match="SAG with ControlNet residuals"):
            eng.run(lat, e, e, e, sag_scale=1.0, **extra, **kw)
    with pytest.raises(ValueError, match="sag_scale"):
        eng.run(lat, e, e, e, sag_scale=-1.0, **kw)
    assert unet.enabled == [] and eng.step_path is None and eng.sag_mass is None


def test_unet_forward_checks_the_mass_buffer():
    from consistentid_amd.unet import HipUNet
    hip = HipUNet.__new__(HipUNet)
    hip.config, hip.W, hip._pag = U.tiny_config("sd15"), {}, ("mid_block.attentions.0.transformer_blocks.0",)
    hip.downs = U.walk(hip.config)[0]
    assert hip.mid_size(32, 32) == (8, 8) and hip.mid_size(24, 16) == (6, 4)
    x = torch.zeros(1, 4, 32, 32)
    good = torch.zeros(1, 64)
    with pytest.raises(NotImplementedError, match="perturbed rows"):
        hip.forward_tokens(x, None, None, 3, pag_rows=1, sag=(good, 0, 1))
    for first, rows in ((-1, 1), (2, 2), (0, 0)):
        with pytest.raises(ValueError, match="sag rows"):
            hip.forward_tokens(x, None, None, 3, sag=(torch.zeros(max(rows, 1), 64), first, rows))
    for bad in (torch.zeros(1, 63), torch.zeros(1, 64, dtype=torch.float16), torch.zeros(2, 64)):
        with pytest.raises(ValueError, match="sag mass"):
            hip.forward_tokens(x, None, None, 3, sag=(bad, 0, 1))


# ----------------------------------------------------------------------------------------------------------- the C ABI
def test_entries_are_declared_exported_and_bound(lib):
    from consistentid_amd import _lib, ops
    names = set(re.findall(r"\b(cid_[a-z0-9_]+)\s*\(", (ROOT / "include" / "cid.h").read_text()))
    assert set(ENTRIES) <= names
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    for n in ENTRIES:
        assert hasattr(lib, n), f"libcid.so does not export {n}"
    assert lib.cid_version() >= 115
    for n in ("attn_colmass", "sag_degrade", "cfg_sag_ddim_step", "cfg_sag_multistep_step", "sag_multistep_step"):
        assert callable(getattr(ops, n))


P = 4096        # a 16-byte-aligned stand-in address: every call below is refused before anything is launched


def test_colmass_refuses_bad_arguments(lib):
    def call(**kw):
        a = {**dict(q=P, ldq=2560, k=P, ldk=2560, mass=P, B=1, N=64, n_keys=64, heads=8, d=160), **kw}
        return lib.cid_attn_colmass_f16(a["q"], a["ldq"], a["k"], a["ldk"], a["mass"], a["B"], a["N"], a["n_keys"], a["heads"], a["d"], None)
    err = lib.cid_last_error
    for name in ("q", "k", "mass"):
        assert call(**{name: None}) == -22 and b"null pointer" in err(), name
        assert call(**{name: P + 8}) == -22 and b"16-byte aligned" in err(), name
    for N in (0, 48, 100, 8192):
        assert call(N=N, n_keys=min(N, 16) or 1) == -22 and b"multiple of 32" in err(), N
    for n_keys in (0, -1, 65):
        assert call(n_keys=n_keys) == -22 and b"n_keys" in err()
    for d in (48, 96, 200, 12):
        assert call(d=d, heads=1) == -22, d
    assert call(ldq=1276) == -22 and call(ldk=640) == -22 and call(B=0) == -22 and call(heads=0) == -22


def test_degrade_refuses_bad_arguments(lib):
    def call(**kw):
        a = {**dict(lat=P, eps=P, mass=P, out=P, coef=P, B=1, C=4, h=8, w=8, hm=2, wm=2), **kw}
        return lib.cid_sag_degrade_f16(a["lat"], a["eps"], a["mass"], a["out"], a["coef"], a["B"], a["C"], a["h"], a["w"], a["hm"], a["wm"], None)
    err = lib.cid_last_error
    for name in ("lat", "eps", "mass", "out", "coef"):
        assert call(**{name: None}) == -22 and b"null pointer" in err(), name
        assert call(**{name: P + 4}) == -22 and b"16-byte aligned" in err(), name
    assert call(h=4) == -22 and b"reflect padding" in err()
    assert call(w=4) == -22 and b"reflect padding" in err()
    assert call(B=0) == -22 and call(C=0) == -22 and call(hm=0) == -22 and call(wm=-1) == -22
    assert call(B=16384, C=4) == -22


def _ddim(lib, **kw):
    a = {**dict(eps=P, lat=P, coef=P, g=5.0, eps_d=P, s=1.0, mask=None, init=None, noise=None, B=1, per=16), **kw}
    return lib.cid_cfg_sag_ddim_step_f16(a["eps"], a["lat"], a["coef"], a["g"], a["eps_d"], a["s"], a["mask"], a["init"],
                                         a["noise"], a["B"], a["per"], None)


def _multistep(lib, cfg):
    def call(**kw):
        a = {**dict(eps=P, lat=P, hist=P, saved=P, z=None, z_rows=0, row=P, g=5.0, eps_d=P, s=1.0, mask=None, init=None,
                    noise=None, B=1, per=16), **kw}
        head = (a["eps"], a["lat"], a["hist"], a["saved"], a["z"], a["z_rows"], a["row"])
        tail = (a["eps_d"], a["s"], a["mask"], a["init"], a["noise"], a["B"], a["per"], None)
        if cfg:
            return lib.cid_cfg_sag_multistep_step_f16(*head, a["g"], *tail)
        return lib.cid_sag_multistep_step_f16(*head, *tail)
    return call


def _common_refusals(lib, call, pointers):
    err = lib.cid_last_error
    for name in pointers + ("eps_d",):
        assert call(**{name: None}) == -22 and b"null pointer" in err(), name
    assert call(eps_d=None, s=0.0) == -22, "a null eps_d is refused at s == 0 too"
    assert call(mask=P) == -22 and b"mask/init/noise" in err()
    assert call(mask=P, init=P) == -22 and call(init=P, noise=P) == -22
    for B in (0, -1):
        assert call(B=B) == -22 and b"multiple of 8" in err()
    assert call(per=0) == -22 and call(per=-8) == -22
    assert call(B=1, per=12) == -22 and b"multiple of 8" in err()
    assert call(B=3, per=4) == -22


def test_ddim_entry_refuses_bad_arguments(lib):
    """what cid_cfg_ddim_step_f16 refuses, and a null eps_d"""
    _common_refusals(lib, lambda **kw: _ddim(lib, **kw), ("eps", "lat", "coef"))


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "single-pass"])
def test_multistep_entries_refuse_bad_arguments(lib, cfg):
    """each entry refuses what its own sibling refuses, and a null eps_d"""
    call = _multistep(lib, cfg)
    _common_refusals(lib, call, ("eps", "lat", "hist", "saved", "row"))
    assert call(z=P, z_rows=0) == -22 and call(z=None, z_rows=2) == -22 and call(z=P, z_rows=-1) == -22
    assert b"z and z_rows" in lib.cid_last_error()
    assert (b"cid_cfg_sag_multistep_step_f16" if cfg else b"cid_sag_multistep_step_f16") in lib.cid_last_error()
    if not cfg:     # the single-pass sibling, cid_multistep_step_f16, also refuses misaligned buffers
        for name in ("eps", "lat", "hist", "saved", "row", "eps_d"):
            assert call(**{name: P + 8}) == -22 and b"16-byte aligned" in lib.cid_last_error(), name
        assert call(z=P + 2, z_rows=1) == -22 and b"16-byte aligned" in lib.cid_last_error()
