"""The face parser on the GPU: the ReLU epilogue of cid_gemm_f16 (act 1) on every path it reaches, the csrc/parsing.hip
kernels against CPU torch, and the whole HipBiSeNet against the fp32 restatement of tests/bisenet_ref.py."""
import pytest
import torch
import torch.nn.functional as F

from bisenet_ref import calibrate, forward, make_image, random_state_dict

pytestmark = pytest.mark.gpu


def _tok(x):
    """NCHW -> token-major [B, H*W, C]"""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


# ----------------------------------------------------------------------------- act = 1 on every GEMM path
# (name, B, cin, cout, H, W, taps, stride, up, centre-tap shortcut, residual): 1x1 on the 128- / 64- / 32-wide and the
# 160-wide tiles, 3x3 stride 1 where act 0 takes the halo / conv3x3.hip kernels, stride 2, nearest-2x + conv, the
# centre-tap 1x1 stride-2 shortcut, and the two-source concat
ACT_CASES = [
    ("1x1_128", 2, 256, 128, 32, 32, 1, 1, 0, False, True),
    ("1x1_64", 1, 128, 64, 64, 64, 1, 1, 0, False, False),
    ("1x1_32", 1, 256, 32, 64, 64, 1, 1, 0, False, False),
    ("1x1_320", 2, 320, 320, 64, 64, 1, 1, 0, False, True),
    ("3x3_s1_halo", 8, 320, 320, 64, 64, 9, 1, 0, False, True),
    ("3x3_s1_128", 1, 64, 64, 128, 128, 9, 1, 0, False, True),
    ("3x3_s2", 2, 128, 256, 64, 64, 9, 2, 0, False, False),
    ("up2x", 1, 128, 128, 16, 16, 9, 1, 1, False, True),
    ("shortcut_s2", 1, 64, 128, 128, 128, 9, 2, 0, True, False),
    ("concat_1x1", 1, 128, 256, 64, 64, 1, 1, 0, False, False),
]


@pytest.mark.parametrize("case", ACT_CASES, ids=[c[0] for c in ACT_CASES])
def test_gemm_act_relu(dev, case):
    from consistentid_amd import ops
    name, B, cin, cout, H, W, taps, stride, up, centre, use_res = case
    g = torch.Generator().manual_seed(cin + cout + H)
    ks = 1 if (taps == 1 or centre) else 3
    x = torch.randn(B, cin, H, W, generator=g).half()
    w = (torch.randn(cout, cin, ks, ks, generator=g) * (ks * ks * cin) ** -0.5).half()
    b = (torch.randn(cout, generator=g) * 0.5).half()
    xi = F.interpolate(x.float(), scale_factor=2, mode="nearest") if up else x.float()
    ref = F.conv2d(xi, w.float(), b.float(), stride=stride, padding=(ks // 2))
    Ho, Wo = ref.shape[2:]
    res = torch.randn(B, cout, Ho, Wo, generator=g).half() if use_res else None
    if res is not None:
        ref = ref + res.float()
    if taps == 1:
        wg = w.reshape(cout, cin)
    elif centre:
        wg = torch.zeros(cout, 9, cin, dtype=torch.float16)
        wg[:, 4] = w.reshape(cout, cin)
        wg = wg.reshape(cout, 9 * cin)
    else:
        wg = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    kw = dict(M=B * Ho * Wo, N=cout, bias=b.to(dev), taps=taps, Hi=H, Wi=W, Ho=Ho, Wo=Wo, stride=stride, up=up,
              res=_tok(res).to(dev) if res is not None else None)
    xt = _tok(x).to(dev)
    if name == "concat_1x1":
        kw.update(x2=xt[..., cin // 2:].contiguous(), c2=cin // 2)
        xt, c1 = xt[..., :cin // 2].contiguous(), cin // 2
    else:
        c1 = cin
    wg = wg.contiguous().to(dev)
    outs = []
    for act in (0, 1):
        out = torch.full((B, Ho * Wo, cout), float("nan"), dtype=torch.float16, device=dev)
        ops.gemm(xt, wg, out, c1=c1, act=act, **kw)
        outs.append(out)
    torch.cuda.synchronize()
    plain, relu = outs[0].cpu(), outs[1].cpu()
    assert torch.isfinite(plain).all() and torch.isfinite(relu).all()
    # the same accumulation, ReLU before the rounding: exactly the ReLU of the act-0 result
    assert torch.equal(relu, torch.relu(plain)), name
    assert (relu < 0).sum() == 0 and (plain < 0).sum() > 0
    refr = torch.relu(_tok(ref))
    err = (relu.float() - refr).norm() / refr.norm()
    assert err < 2e-3, f"{name}: rel_l2 {err:.2e}"


# ----------------------------------------------------------------------------- stem
@pytest.mark.parametrize("B,H,W", [(1, 512, 512), (2, 96, 160)])
def test_parse_stem(dev, B, H, W):
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(H + W)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.1
    x = img.permute(0, 3, 1, 2).float() / 255
    x = (x - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    ref = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=3)), 3, 2, 1)
    out = torch.full((B, (H // 4) * (W // 4), 64), float("nan"), dtype=torch.float16, device=dev)
    ops.parse_stem(img.to(dev), out, w.permute(0, 2, 3, 1).contiguous().to(dev), b.to(dev))
    torch.cuda.synchronize()
    r = _tok(ref)
    got = out.cpu().float()
    assert torch.isfinite(got).all()
    assert (got - r).abs().max() / r.abs().max() < 1e-3        # fp16 rounding of the pooled fp32 values


# ----------------------------------------------------------------------------- pooled branches
def test_chan_mean_gate_affine(dev):
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(5)
    B, HW, C = 2, 1024, 256
    x = (torch.randn(B, HW, C, generator=g) + 0.5).half()
    m = torch.empty(B, C, dtype=torch.float32, device=dev)
    ops.chan_mean(x.to(dev), m, B=B, HW=HW, C_=C)
    ref_m = x.double().mean(1)
    torch.cuda.synchronize()
    assert (m.cpu().double() - ref_m).abs().max() < 1e-5
    # one layer + ReLU (conv_avg), one layer + sigmoid (ARM), two layers + sigmoid (FFM)
    w1 = torch.randn(128, C, generator=g) * C ** -0.5
    b1 = torch.randn(128, generator=g) * 0.1
    w2 = torch.randn(C, 128, generator=g) * 128 ** -0.5
    mm = m.cpu()
    for act, use_w2, ref in ((1, False, torch.relu(mm @ w1.T + b1)), (2, False, torch.sigmoid(mm @ w1.T + b1)),
                             (0, False, mm @ w1.T + b1), (2, True, torch.sigmoid(torch.relu(mm @ w1.T + b1) @ w2.T))):
        n = w2.shape[0] if use_w2 else w1.shape[0]
        out = torch.empty(B, n, dtype=torch.float32, device=dev)
        ops.chan_gate(m, out, w1.to(dev), b1.to(dev), w2.to(dev) if use_w2 else None, act=act)
        torch.cuda.synchronize()
        assert (out.cpu() - ref).abs().max() < 1e-5, (act, use_w2)
    s = torch.rand(B, C, generator=g)
    t = torch.randn(B, C, generator=g)
    res = torch.randn(B, HW, C, generator=g).half()
    for kind in ("t", "res", "self"):
        out = torch.empty(B, HW, C, dtype=torch.float16, device=dev)
        kw = {"t": dict(t=t.to(dev)), "res": dict(res=res.to(dev)), "self": {}}[kind]
        ops.chan_affine(x.to(dev), s.to(dev), out, B=B, HW=HW, C_=C, **kw)
        add = {"t": t[:, None, :], "res": res.float(), "self": x.float()}[kind]
        ref = (x.float() * s[:, None, :] + add).half()
        torch.cuda.synchronize()
        assert (out.cpu().float() - ref.float()).abs().max() <= 2 ** -10 * ref.float().abs().max(), kind


# ----------------------------------------------------------------------------- head
@pytest.mark.parametrize("B,h,w,H,W", [(2, 24, 40, 96, 160), (1, 64, 64, 512, 512)])
def test_parse_head(dev, B, h, w, H, W):
    from consistentid_amd import ops
    g = torch.Generator().manual_seed(h * w)
    lg = (torch.randn(B, h * w, 32, generator=g) * 3).half()
    lg[:, :, 19:] = 100          # padding channels beyond ncls must never win
    lg[0, 0, 3] = lg[0, 0, 7] = 50   # an exact tie at the corner pixel: the first maximum wins
    labels = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    up = torch.empty(B, 19, H, W, dtype=torch.float32, device=dev)
    ops.parse_head(lg.to(dev), labels, ncls=19, B=B, h=h, w=w, H=H, W=W, logits_out=up)
    nchw = lg[..., :19].float().reshape(B, h, w, 19).permute(0, 3, 1, 2)
    ref = F.interpolate(nchw, (H, W), mode="bilinear", align_corners=True)
    torch.cuda.synchronize()
    got_up, got_lab = up.cpu(), labels.cpu().long()
    assert (got_up - ref).abs().max() < 1e-4 * ref.abs().max()
    assert got_lab[0, 0, 0] == 3
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(got_lab[sure], ref.argmax(1)[sure])
    assert torch.equal(got_lab, got_up.argmax(1))      # argmax of the logits it wrote, first maximum included


# ----------------------------------------------------------------------------- whole network
LOGIT_TOL = 1e-2          # relative L2 of the upsampled logits, fp16 engine vs the fp32 restatement
MARGIN = 0.05             # labels must agree wherever the fp32 top-1 / top-2 gap exceeds MARGIN x the logits' RMS


@pytest.fixture(scope="module")
def conditioned_net():
    sd = random_state_dict(seed=11)
    calibrate(sd, make_image(1, 512, 512, seed=100))
    return sd


@pytest.mark.parametrize("B", [1, 2])
def test_bisenet_end_to_end(dev, conditioned_net, B):
    from consistentid_amd.face_parsing import HipBiSeNet
    sd = conditioned_net
    net = HipBiSeNet(sd, device=dev)
    img = make_image(B, 512, 512, seed=200 + B)
    labels, up = net(img, logits=True)
    torch.cuda.synchronize()
    ref = forward(sd, img)
    got = up.cpu()
    assert torch.isfinite(got).all()
    err = float((got - ref).norm() / ref.norm())
    top2 = ref.topk(2, dim=1).values
    rms = ref.pow(2).mean().sqrt()
    sure = (top2[:, 0] - top2[:, 1]) > MARGIN * rms
    ref_lab = ref.argmax(1)
    lab = labels.cpu().long()
    agree = float((lab == ref_lab).float().mean())
    # for scale: the same restatement run in fp16 with stock PyTorch kernels on this GPU
    arm = forward({k: v.to(dev) for k, v in sd.items()}, img.to(dev), torch.float16).float().cpu()
    err_arm = float((arm - ref).norm() / ref.norm())
    print(f"[face parsing] B={B}: logits rel_l2 {err:.2e} (stock fp16 arm {err_arm:.2e}), label agreement {agree:.5f}, "
          f"{float(sure.float().mean()):.4f} of the pixels past the margin, classes used {ref_lab.unique().numel()}")
    assert err < LOGIT_TOL
    assert torch.equal(lab[sure], ref_lab[sure])
    assert torch.equal(lab, got.argmax(1))
    # labels only: same answer without the logits buffer, and from PIL input through the reference's resize
    assert torch.equal(net(img).cpu(), labels.cpu())
    from PIL import Image
    pil = [Image.fromarray(img[i].numpy()).resize((300, 260)) for i in range(B)]
    from consistentid_amd.face_parsing import to_pixels
    assert torch.equal(net(pil).cpu(), net(to_pixels(pil)).cpu())


def test_bisenet_non_square(dev, conditioned_net):
    from consistentid_amd.face_parsing import HipBiSeNet
    net = HipBiSeNet(conditioned_net, device=dev)
    img = make_image(1, 256, 384, seed=7)
    labels, up = net(img, logits=True)
    ref = forward(conditioned_net, img)
    torch.cuda.synchronize()
    assert labels.shape == (1, 256, 384)
    assert float((up.cpu() - ref).norm() / ref.norm()) < LOGIT_TOL
