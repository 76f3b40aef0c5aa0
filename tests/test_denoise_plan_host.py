"""The denoise engine's host-side phases without a GPU or the library: the embed-row selectors of every schedule entry,
the ControlNet argument preparation of the pipeline call, the keep table of a plain net, the ``eta`` refusals and the key
of what a captured step reads of the UNet and the ControlNets."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch


# --------------------------------------------------------------------------- step rows
@pytest.mark.parametrize("has_null_post", [False, True])
@pytest.mark.parametrize("start_merge_step", [0, 1, 10])
@pytest.mark.parametrize("first_step", [0, 1])
def test_step_rows_follow_the_reference_loop(first_step, start_merge_step, has_null_post):
    """K/V rows [0,B) null, [B,2B) text-only, [2B,3B) augmented, [3B,4B) null-post (UNet); [0,B) text-only, [B,2B)
    augmented (ControlNet).  The reference's ``for i, t in enumerate(timesteps)`` runs over the truncated list, so its i
    is the schedule entry minus ``first_step``; skipped entries follow the same formula."""
    from consistentid_amd.denoise import step_rows
    B, n_ts = 2, 4
    rows = step_rows(n_ts, first_step, start_merge_step, B, has_null_post)
    assert rows.unet.dtype == rows.controlnet.dtype == torch.int32
    assert tuple(rows.unet.shape) == (n_ts, 2 * B) and tuple(rows.controlnet.shape) == (n_ts, B)
    assert rows.unet.device.type == rows.controlnet.device.type == "cpu"
    for entry in range(n_ts):
        merged = entry - first_step > start_merge_step
        b = list(range(B))
        if merged:
            uncond = [(3 * B if has_null_post else 0) + k for k in b]
            want_unet, want_cn = uncond + [2 * B + k for k in b], [B + k for k in b]
        else:
            want_unet, want_cn = b + [B + k for k in b], b
        assert rows.unet[entry].tolist() == want_unet, (entry, rows.unet[entry])
        assert rows.controlnet[entry].tolist() == want_cn, (entry, rows.controlnet[entry])
        assert bool(rows.merged[entry]) == merged
    assert step_rows(n_ts, first_step, start_merge_step, B, has_null_post, controlnet=False).controlnet is None


# --------------------------------------------------------------------------- control arguments
class _Net:
    """stands in for a HipControlNet: the preparation only looks at the pipeline's controlnet to tell one net from several"""


def _multi(n):
    from consistentid_amd.controlnet import HipMultiControlNet
    multi = HipMultiControlNet.__new__(HipMultiControlNet)
    multi.nets = [_Net() for _ in range(n)]
    return multi


SIZE = (16, 24)


def test_control_arguments_of_a_plain_net():
    from PIL import Image
    from consistentid_amd.controlnet import prepare_control_arguments
    net, img = _Net(), torch.rand(1, 3, *SIZE)
    kw = prepare_control_arguments(net, img, 0.5, 0.0, 0.75, SIZE)
    assert kw["controlnet"] is net and kw["control_image"] is img
    assert (kw["conditioning_scale"], kw["control_guidance_start"], kw["control_guidance_end"]) == (0.5, 0.0, 0.75)
    # a list of one PIL image is that image, resized to the target size (CN :267-280); of lists of scales the first counts
    pil = Image.fromarray(np.full((9, 10, 3), 255, np.uint8))
    kw = prepare_control_arguments(net, [pil], [0.3, 0.9], [0.1], (0.8, 0.9), SIZE)
    assert kw["controlnet"] is net and tuple(kw["control_image"].shape) == (1, 3, *SIZE)
    assert torch.equal(kw["control_image"], torch.ones(1, 3, *SIZE))
    assert (kw["conditioning_scale"], kw["control_guidance_start"], kw["control_guidance_end"]) == (0.3, 0.1, 0.8)
    with pytest.raises(NotImplementedError, match="MultiControlNet: several control images need"):
        prepare_control_arguments(net, [img, img], 0.5, 0.0, 1.0, SIZE)
    with pytest.raises(NotImplementedError, match=r"^control_image: one PIL image .* numpy arrays are not taken"):
        prepare_control_arguments(net, np.zeros((1, 3, *SIZE), np.float32), 0.5, 0.0, 1.0, SIZE)
    with pytest.raises(NotImplementedError, match="numpy arrays are not taken"):
        prepare_control_arguments(net, [img], 0.5, 0.0, 1.0, SIZE)          # a list of one TENSOR is not an image
    # no control image: no net runs; a control image without a net is an error
    assert prepare_control_arguments(net, None, 0.5, 0.0, 1.0, SIZE)["controlnet"] is None
    assert prepare_control_arguments(None, None, 0.5, 0.0, 1.0, SIZE)["controlnet"] is None
    with pytest.raises(ValueError, match="control_image given but the pipeline was built without a controlnet"):
        prepare_control_arguments(None, img, 0.5, 0.0, 1.0, SIZE)


def test_control_arguments_of_several_nets():
    from consistentid_amd.controlnet import prepare_control_arguments
    multi, imgs = _multi(2), [torch.rand(1, 3, *SIZE), torch.rand(2, 3, *SIZE)]
    kw = prepare_control_arguments(multi, imgs, 0.5, 0.25, [0.75, 1.0], SIZE)         # a float scale goes to every net
    assert kw["controlnet"] is multi and all(a is b for a, b in zip(kw["control_image"], imgs))
    assert kw["conditioning_scale"] == [0.5, 0.5]
    assert (kw["control_guidance_start"], kw["control_guidance_end"]) == ([0.25, 0.25], [0.75, 1.0])
    assert prepare_control_arguments(multi, imgs, (0.5, 0.8), 0.0, 1.0, SIZE)["conditioning_scale"] == [0.5, 0.8]
    with pytest.raises(ValueError, match="control_image has 1 entries for 2 ControlNets"):
        prepare_control_arguments(multi, imgs[0], 0.5, 0.0, 1.0, SIZE)
    with pytest.raises(ValueError, match="control_image has 3 entries for 2 ControlNets"):
        prepare_control_arguments(multi, imgs + imgs[:1], 0.5, 0.0, 1.0, SIZE)
    with pytest.raises(ValueError, match="controlnet_conditioning_scale has 3 entries for 2 ControlNets"):
        prepare_control_arguments(multi, imgs, [0.1, 0.2, 0.3], 0.0, 1.0, SIZE)
    with pytest.raises(ValueError, match="controlnet_conditioning_scale has 3 entries for 2 ControlNets"):
        prepare_control_arguments(multi, None, [0.1, 0.2, 0.3], 0.0, 1.0, SIZE)        # refused without an image too
    with pytest.raises(ValueError, match="3 entries for 2 ControlNets"):
        prepare_control_arguments(multi, imgs, 0.5, [0.0, 0.1, 0.2], 1.0, SIZE)
    with pytest.raises(NotImplementedError, match=r"^control_image\[1\]: one PIL image .* numpy arrays are not taken"):
        prepare_control_arguments(multi, [imgs[0], np.zeros((1, 3, *SIZE), np.float32)], 0.5, 0.0, 1.0, SIZE)


@pytest.mark.parametrize("first_step", [0, 1])
def test_keep_table_of_a_plain_net_is_the_reference_formula(first_step):
    """CN :364-371 with one net, over the executed steps; skipped entries keep 0"""
    from consistentid_amd.controlnet import active_nets, controlnet_keep_table, prepare_control_arguments
    n, end = 4, 0.75
    kw = prepare_control_arguments(_Net(), torch.rand(1, 3, *SIZE), 0.5, 0.0, end, SIZE)
    start, end = kw["control_guidance_start"], kw["control_guidance_end"]
    keep = controlnet_keep_table(n, [start], [end], first_step)
    want = [0.0] * first_step + [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]
    assert keep == [[v] for v in want] and want[first_step:] == [1.0, 1.0, 1.0, 0.0]
    assert [active_nets(r) for r in keep] == [()] * first_step + [(0,), (0,), (0,), ()]
    # the engine's own wiring of it: a plain net is a list of one, the formula counts the executed steps of the schedule
    from consistentid_amd.denoise import DenoiseEngine, step_rows
    net = SimpleNamespace(context_addresses=lambda: (), set_context=lambda ehs, num_tokens: None, cond_embedding=lambda img: img)
    eng = DenoiseEngine(SimpleNamespace(device="cpu"), None, use_graph=False)
    n_ts, embeds = n + first_step, torch.zeros(2, 1, 4)
    plan = eng._control_plan(net, torch.zeros(1, 3, 8, 8), 0.5, start, end, embeds, embeds,
                             step_rows(n_ts, first_step, 0, 2, False), torch.zeros(n_ts), first_step, temb_table=False)
    assert plan.keep == keep and plan.nets == [net] and plan.fold == 0.5 and plan.scale_column is None


# --------------------------------------------------------------------------- eta
def _messages(sch, eta, variance_noise):
    """the refusal of the pipeline's pre-loop and of the engine's run for the same arguments"""
    from consistentid_amd import pipeline
    pipe = pipeline.ConsistentIDStableDiffusionPipeline(SimpleNamespace(device="cpu"), scheduler=sch, use_graph=False)
    lat = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError) as from_pipe:
        pipe._variance_noise(eta, None, variance_noise, lat, 4)
    with pytest.raises(ValueError) as from_engine:
        pipe._engine.run(lat, None, None, None, num_inference_steps=4, guidance_scale=5.0, start_merge_step=0, eta=eta,
                         variance_noise=variance_noise)
    assert str(from_pipe.value) == str(from_engine.value)
    return str(from_pipe.value)


def test_eta_refusals_are_the_same_from_pipeline_and_engine():
    from consistentid_amd import scheduler
    noise = torch.zeros(4, 1, 4, 8, 8)
    for sch in (scheduler.PNDMScheduler(), scheduler.EulerDiscreteScheduler()):
        msg = _messages(sch, 0.5, noise)
        assert msg.startswith(f"eta = 0.5: only DDIMScheduler has an eta term ({type(sch).__name__} is deterministic)")
    assert _messages(scheduler.DDIMScheduler(), -0.5, noise) == "eta = -0.5: DDIM's eta is in [0, 1]"
    for sch in (scheduler.DDIMScheduler(), scheduler.PNDMScheduler()):
        assert _messages(sch, 0.0, noise) == "variance_noise without eta: the noise term has the coefficient eta * sigma_t"


# --------------------------------------------------------------------------- what a captured step reads
class _Obj:
    """stands in for a HipUNet / HipControlNet: a serial from one counter, an epoch, K/V buffers that ``set_context`` moves when
    the row count changes (and then counts in the epoch), as unet.py does.  ``pool`` plays the caching allocator: a freed
    address is handed out again for the next request of the same size."""
    _serials = iter(range(1, 1000))

    def __init__(self, pool, addresses=None):
        self.serial, self.epoch, self.pool, self.rows = next(self._serials), 0, pool, None
        self.addr = addresses

    def set_context(self, rows):
        if rows != self.rows:
            if self.rows is not None:
                self.pool.setdefault(self.rows, []).append(self.addr)
            free = self.pool.get(rows)
            self.addr = free.pop() if free else (0x1000 * self.serial + rows,)
            self.rows, self.epoch = rows, self.epoch + 1

    def load_adapter_modules(self):
        self.epoch += 1

    def context_addresses(self):
        return (*self.addr, 77, 4)


def test_captured_reads_tell_objects_orders_moves_and_epochs_apart():
    from consistentid_amd.denoise import captured_reads
    unet, a, b = _Obj({}, (0x100,)), _Obj({}, (0x200,)), _Obj({}, (0x200,))
    assert a.context_addresses() == b.context_addresses()
    assert captured_reads(unet, [a]) == captured_reads(unet, [a]) == captured_reads(unet, (a,))
    assert captured_reads(unet, [a, b]) == captured_reads(unet, [a, b])
    assert captured_reads(unet, [a]) != captured_reads(unet, [b])             # A against B at identical addresses and shapes
    assert captured_reads(unet, [a, b]) != captured_reads(unet, [b, a])
    assert captured_reads(unet, []) != captured_reads(unet, [a]) != captured_reads(unet, [a, b])
    before = captured_reads(unet, [a])
    a.load_adapter_modules()                                                  # a host-side launch argument changed
    assert captured_reads(unet, [a]) != before and captured_reads(unet, [a])[0] == before[0]
    before = captured_reads(unet, [a])
    unet.load_adapter_modules()
    assert captured_reads(unet, [a]) != before and captured_reads(unet, [a])[1] == before[1]


def test_captured_reads_after_a_shared_unet_moved_and_moved_back():
    """One UNet under two engines: engine 1 captures at 6 rows (B = 2); engine 2 sets 3 rows, then 6 again, and the
    allocator hands the first address out a second time.  The addresses are those engine 1 captured with, the key is not."""
    from consistentid_amd.denoise import captured_reads
    unet = _Obj({})
    unet.set_context(6)
    engine1 = captured_reads(unet, [])
    unet.set_context(6)                                     # engine 1 again, same shapes: nothing moved
    assert captured_reads(unet, []) == engine1
    unet.set_context(3)                                     # engine 2 at B = 1
    engine2 = captured_reads(unet, [])
    assert engine2 != engine1
    unet.set_context(6)                                     # engine 2 at B = 2
    assert unet.context_addresses() == engine1[0][2]        # (moved back)
    assert captured_reads(unet, []) not in (engine1, engine2)
    unet.set_context(6)                                     # engine 1 at B = 2: ``set_context`` keeps the buffers
    assert unet.context_addresses() == engine1[0][2] and captured_reads(unet, []) != engine1


def test_captured_reads_hold_nothing_the_step_table_carries():
    """the function sees the objects only: scales, merge step, ``first_step`` and the guidance windows cannot reach it, and
    the key is (serial, epoch, addresses) per object and nothing else"""
    import inspect
    from consistentid_amd.denoise import captured_reads
    assert list(inspect.signature(captured_reads).parameters) == ["unet", "nets"]
    unet, a = _Obj({}, (0x100, 0x180)), _Obj({}, (0x200,))
    assert captured_reads(unet, [a]) == ((unet.serial, 0, (0x100, 0x180, 77, 4)), (a.serial, 0, (0x200, 77, 4)))
    for name in ("conditioning_scale", "fold", "start_merge_step", "first_step", "keep", "guidance_scale"):
        setattr(a, name, 0.25)
        setattr(unet, name, 3)
    assert captured_reads(unet, [a]) == ((unet.serial, 0, (0x100, 0x180, 77, 4)), (a.serial, 0, (0x200, 77, 4)))
